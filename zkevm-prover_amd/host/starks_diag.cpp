// The prover's diagnostics (starks.hpp Probe, Checks): the probe, the
// constraint check and its naming, the diagnosis of a grand product that does
// not close, the trace audit and the connection checks.  None of them is part
// of the proof schedule (starks.cpp), which calls them at its hooks.
#include "starks.hpp"
#include "zkgpu_audit_format.hpp"

namespace zkgpu_host {

// One library call that reports into a device block of k words of its own:
// the block lives for the call, its words end in h; not 0: `why` is the
// library's text
template <class Call> static int result_block(uint64_t *h, uint32_t k, std::string &why, Call call)
{
    void *dev = nullptr;
    int rc = zkgpu_dev_malloc(&dev, k * 8);
    if (!rc) rc = call((uint64_t *)dev);
    if (!rc) rc = zkgpu_memcpy_d2h(h, dev, k * 8);
    why = rc ? zkgpu_last_error() : "";
    (void)zkgpu_dev_free(dev);
    return rc;
}

// ---------------------------------------------------------------- probe
int Probe::set(Starks &s, const uint64_t *rows_n, uint32_t n_rows_n, const uint64_t *rows_ext, uint32_t n_rows_ext)
{
    clear();
    if (!n_rows_n && !n_rows_ext) return 0;
    if ((n_rows_n && !rows_n) || (n_rows_ext && !rows_ext)) return fail("probe_set: null row list");
    if (n_rows_n > ZKGPU_PROBE_MAX_ROWS || n_rows_ext > ZKGPU_PROBE_MAX_ROWS)
        return fail("probe_set: %u / %u sampled rows, at most %u per domain", n_rows_n, n_rows_ext,
                    ZKGPU_PROBE_MAX_ROWS);
    std::vector<uint64_t> base[2] = {std::vector<uint64_t>(rows_n, rows_n + n_rows_n),
                                     std::vector<uint64_t>(rows_ext, rows_ext + n_rows_ext)};
    for (int e = 0; e < 2; e++) {
        std::sort(base[e].begin(), base[e].end());
        base[e].erase(std::unique(base[e].begin(), base[e].end()), base[e].end());
        const uint64_t dom = e ? s.NE : s.N;
        if (!base[e].empty() && base[e].back() >= dom)
            return fail("probe_set: row %llu is outside the %s domain (%llu rows)",
                        (unsigned long long)base[e].back(), e ? "extended" : "n", (unsigned long long)dom);
    }
    std::vector<std::vector<uint64_t>> lists;  // row list of each record
    auto add = [&](uint32_t point, uint32_t after, uint32_t sec, uint32_t ncols, std::vector<uint64_t> rows) {
        Rec p;
        p.r = {point, after, sec, ncols, (uint64_t)rows.size(), 0, 0};
        at[point][after].push_back((uint32_t)recs.size());
        recs.push_back(p);
        lists.push_back(std::move(rows));
    };
    const uint32_t n_scal = 24 + 3 * s.info.n_ev;
    struct Point {
        uint32_t point;
        const Prog *prog;  // null: a stage step with one after-record
        bool ext, present;
        uint32_t sec;
        const char *name;
    };
    const Point points[ZKGPU_PROBE_POINTS] = {
        {ZKGPU_PROBE_STEP2, &s.step2, false, true, 0, "step2"},
        {ZKGPU_PROBE_H1H2, nullptr, false, s.info.n_pu != 0, SEC_CM2_N, "h1h2"},
        {ZKGPU_PROBE_STEP3PREV, &s.step3prev, false, true, 0, "step3prev"},
        {ZKGPU_PROBE_Z, nullptr, false, true, SEC_CM3_N, "z"},
        {ZKGPU_PROBE_STEP3, &s.step3, false, !s.step3.instr.empty(), 0, "step3"},
        {ZKGPU_PROBE_STEP42NS, &s.step42ns, true, true, 0, "step42ns"},
        {ZKGPU_PROBE_QSPLIT, nullptr, true, true, SEC_CM4_2NS, "qsplit"},
        {ZKGPU_PROBE_STEP52NS, &s.step52ns, true, true, 0, "step52ns"},
    };
    for (const Point &pt : points) {
        if (!pt.present) continue;
        add(pt.point, 0, ZKGPU_PROBE_SCALARS, n_scal, {0});
        const uint64_t dom = pt.ext ? s.NE : s.N;
        if (!pt.prog) {
            add(pt.point, 1, pt.sec, s.S.ncols[pt.sec], base[pt.ext]);
            continue;
        }
        // the sections the program reads / stores to, and every row shift it uses with each
        std::vector<int32_t> shifts[SEC_COUNT];
        bool reads[SEC_COUNT] = {false}, stores[SEC_COUNT] = {false};
        auto use = [&](uint32_t k, bool store) -> int {
            if (k >= pt.prog->opnd.size()) return fail("probe_set: %s names operand %u of %zu", pt.name, k,
                                                       pt.prog->opnd.size());
            const zxp_operand &o = pt.prog->opnd[k];
            if (o.kind != ZXP_COL && o.kind != ZXP_COL3) return 0;
            if (o.a >= SEC_COUNT) return fail("probe_set: %s names section %u", pt.name, o.a);
            if ((o.a >= SEC_CM1_2NS) != pt.ext)
                return fail("probe_set: %s %s section %u of the other domain: its rows are not the sampled rows'",
                            pt.name, store ? "writes" : "reads", o.a);
            (store ? stores : reads)[o.a] = true;
            shifts[o.a].push_back((int32_t)o.c);
            return 0;
        };
        for (const zxp_instr &in : pt.prog->instr)
            if (use(in.a, false) || (in.op != ZXP_COPY && use(in.b, false)) || use(in.dst, true)) {
                clear();
                return -1;
            }
        std::vector<uint64_t> rows[SEC_COUNT];
        for (uint32_t sec = 0; sec < SEC_COUNT; sec++) {
            if (!reads[sec] && !stores[sec]) continue;
            shifts[sec].push_back(0);
            for (uint64_t r : base[pt.ext])
                for (int32_t sh : shifts[sec]) rows[sec].push_back((r + (uint64_t)(int64_t)sh) & (dom - 1));
            std::sort(rows[sec].begin(), rows[sec].end());
            rows[sec].erase(std::unique(rows[sec].begin(), rows[sec].end()), rows[sec].end());
        }
        for (uint32_t after = 0; after < 2; after++)
            for (uint32_t sec = 0; sec < SEC_COUNT; sec++)
                if (after ? stores[sec] : reads[sec]) add(pt.point, after, sec, s.S.ncols[sec], rows[sec]);
    }
    // payload: every record's row list (and the scalars' values), then the gathered values
    uint64_t cur = 0;
    for (size_t i = 0; i < recs.size(); i++) {
        zkgpu_probe_rec &r = recs[i].r;
        r.rows_off = cur;
        cur += r.n_rows;
        if (r.section == ZKGPU_PROBE_SCALARS) {
            r.vals_off = cur;
            cur += r.ncols;
        }
    }
    gather0 = cur;
    std::map<std::vector<uint64_t>, uint64_t> seen;  // identical row lists share one device copy
    std::vector<uint64_t> dev_rows;
    for (size_t i = 0; i < recs.size(); i++) {
        Rec &p = recs[i];
        if (p.r.section == ZKGPU_PROBE_SCALARS) continue;
        p.stage = stage_words;
        p.r.vals_off = gather0 + stage_words;
        stage_words += p.r.n_rows * p.r.ncols;
        auto it = seen.find(lists[i]);
        if (it == seen.end()) {
            it = seen.emplace(lists[i], (uint64_t)dev_rows.size()).first;
            dev_rows.insert(dev_rows.end(), lists[i].begin(), lists[i].end());
        }
        p.rows_dev = it->second;
    }
    payload.assign(gather0 + stage_words, 0);
    for (size_t i = 0; i < recs.size(); i++)
        std::copy(lists[i].begin(), lists[i].end(), payload.begin() + recs[i].r.rows_off);
    void *stage = nullptr, *rows = nullptr;
    if (zkgpu_dev_malloc(&stage, stage_words * 8) || zkgpu_dev_malloc(&rows, dev_rows.size() * 8)) {
        if (stage) (void)zkgpu_dev_free(stage);
        const double mb = (double)(stage_words + dev_rows.size()) * 8 / 1e6;
        clear();
        return fail("probe_set: the probe's device block (%.1f MB) could not be allocated: %s; the probe is off",
                    mb, zkgpu_last_error());
    }
    d_stage = (uint64_t *)stage;
    d_rows = (uint64_t *)rows;
    if (zkgpu_memcpy_h2d(d_rows, dev_rows.data(), dev_rows.size() * 8)) {
        clear();
        return fail("probe_set: %s; the probe is off", zkgpu_last_error());
    }
    return 0;
}

// after the proof's last kernel and its total timer: the one copy to the host
int Probe::readback(Starks &s)
{
    if (recs.empty()) return 0;
    const auto t = Starks::clk::now();
    CK(zkgpu_memcpy_d2h(payload.data() + gather0, d_stage, stage_words * 8));
    s.timers.emplace_back("ZKGPU_PROBE_READBACK",
                          std::chrono::duration<double, std::milli>(Starks::clk::now() - t).count());
    valid = true;
    return 0;
}

// ---- constraint check (include/zkgpu_stark.h zkgpu_stark_check_*): the
// quotient program on the trace domain, before stage 3's commit.  The
// combination C that step42ns forms before its "x ZI" is zero on every
// row of <omega_n> iff the trace satisfies every identity, so the same
// instruction list over the n-domain sections (nd_opnd: step42ns's
// operands rewritten by zkgpu_zxp_to_n_domain) names the rows that break
// the AIR at 1 / 2^blowup of the quotient's rows.  Its 3 output columns
// borrow the head of q (dead until stage 4); the rows that are not zero
// come from zkgpu_nonzero_rows_dev into a 20-word device block of the
// check's own (outside the memory plan, as the probe's).
int Checks::set(Starks &s, uint32_t m)
{
    if (m > ZKGPU_CHECK_STOP) return fail("check_set: unknown mode %u", m);
    mode = ZKGPU_CHECK_OFF;
    std::string why;
    if (m != ZKGPU_CHECK_OFF && !prepare(s, why)) return fail("check_set: %s; the check is off", why.c_str());
    mode = m;
    return 0;
}
// the n-domain rewrite of step42ns, once, for the check and the naming, and (`block`) the check's
// device block; false: `why` says what was refused (the mode is the caller's business: the audit
// uses the check without setting one)
bool Checks::prepare(Starks &s, std::string &why, bool block)
{
    if (nd_opnd.empty()) {
        const Prog &p = s.step42ns;
        std::vector<zxp_operand> o(p.opnd.size() + 1);
        if (zkgpu_zxp_to_n_domain(o.data(), p.instr.data(), (uint32_t)p.instr.size(), p.opnd.data(),
                                  (uint32_t)p.opnd.size(), s.eb)) {
            why = std::string("step42ns: ") + zkgpu_last_error();
            return false;
        }
        o.resize(p.opnd.size());
        nd_opnd.swap(o);
    }
    if (block && !dev) {
        void *v = nullptr;
        if (zkgpu_dev_malloc(&v, (4 + ZKGPU_CHECK_MAX_ROWS) * 8)) {
            why = zkgpu_last_error();
            return false;
        }
        dev = (uint64_t *)v;
    }
    return true;
}

// between the last stage-3 program and stage 3's commit: every n-domain
// section is alive under both memory plans.  The combination challenge
// (challenge 4) comes from root 3, which does not exist yet, so the check
// takes its own: the getField of a COPY of the transcript as it stands
// (challenges 2 and 3 drawn); the proof's transcript is not touched.
int Checks::run(Starks &s, const Transcript &tr, const uint64_t ch[24])
{
    if (mode == ZKGPU_CHECK_OFF) return 0;
    if (queue(s, tr, ch, "ZKGPU_CHECK_CONSTRAINTS")) return -1;
    if (mode == ZKGPU_CHECK_REPORT) {
        pending = true;
        return 0;
    }
    if (readback()) return -1;  // STOP: the one synchronisation
    if (res.n_bad) {
        // the terms that fail at the first row, up to 8 (with naming on)
        std::string tail;
        if (names_on) {
            const std::vector<uint32_t> &ids = names_ids[0];
            if (!ids.empty()) tail = "; failing terms there:";
            for (size_t k = 0; k < ids.size() && k < 8; k++) tail += " " + std::to_string(ids[k]);
            if (ids.size() > 8) tail += " and " + std::to_string(ids.size() - 8) + " more";
            if (!ids.empty()) tail += " (zkgpu_stark_check_named)";
        }
        return fail("constraint check: %llu of the 2^%u = %llu rows of the trace break the AIR; the first is row "
                    "%llu (zkgpu_stark_check_result lists the lowest %u)%s",
                    (unsigned long long)res.n_bad, s.info.n_bits, (unsigned long long)s.N,
                    (unsigned long long)res.rows[0], (unsigned)ZKGPU_CHECK_MAX_ROWS, tail.c_str());
    }
    return 0;
}
// the check's launches (and, with naming on, the names') under one timer line; nothing is read back
int Checks::queue(Starks &s, const Transcript &tr, const uint64_t ch[24], const char *timer)
{
    s.tstart();
    const Prog &p = s.step42ns;
    const uint64_t N = s.N;
    Transcript fork = tr;
    uint64_t chk[24];
    memcpy(chk, ch, sizeof chk);
    fork.get_field(chk + 12);
    memcpy(res.alpha, chk + 12, 24);
    zkgpu_sections T = s.S;
    const uint32_t pairs[4][2] = {{SEC_CM1_2NS, SEC_CM1_N}, {SEC_CM2_2NS, SEC_CM2_N}, {SEC_CM3_2NS, SEC_CM3_N},
                                  {SEC_CONST_2NS, SEC_CONST_N}};
    for (const auto &pr : pairs) {
        T.sec[pr[0]] = s.S.sec[pr[1]];
        T.ld[pr[0]] = N;
        T.ncols[pr[0]] = s.S.ncols[pr[1]];
    }
    uint64_t *c = s.S.sec[SEC_Q_2NS];  // its first 3 N words, ld N
    T.ld[SEC_Q_2NS] = N;
    const uint64_t ev0[3] = {0, 0, 0};
    CK(zkgpu_zxp_eval_dev(p.instr.data(), (uint32_t)p.instr.size(), nd_opnd.data(), (uint32_t)nd_opnd.size(),
                          p.n_tmp1 ? p.n_tmp1 : 1, p.n_tmp3 ? p.n_tmp3 : 1, &T, s.info.n_bits, chk,
                          s.publics.data(), (uint32_t)s.publics.size(), ev0, 0, nullptr, nullptr, 0, 1));
    CK(zkgpu_nonzero_rows_dev(dev, c, N, 3, N, ZKGPU_CHECK_MAX_ROWS));
    // C at the first failing row (a row index past the domain -- none failed -- reads 0)
    CK(zkgpu_gather_rows_dev(dev + 1 + ZKGPU_CHECK_MAX_ROWS, c, N, 3, dev + 1, 1));
    if (names_on) {
        // every term of C at the listed rows: the tapped program over the same sections, its
        // 3K output columns the names' block (ld 16), the row list the check's own on the device
        T.sec[SEC_Q_2NS] = names_dev;
        T.ld[SEC_Q_2NS] = ZKGPU_CHECK_MAX_ROWS;
        T.ncols[SEC_Q_2NS] = 3 * (uint32_t)names_terms.size();
        CK(zkgpu_zxp_eval_rows_dev(names_instr.data(), (uint32_t)names_instr.size(), names_opnd.data(),
                                   (uint32_t)names_opnd.size(), p.n_tmp1 ? p.n_tmp1 : 1, p.n_tmp3 ? p.n_tmp3 : 1, &T,
                                   s.info.n_bits, chk, s.publics.data(), (uint32_t)s.publics.size(), ev0, 0, nullptr,
                                   nullptr, 0, 1, dev + 1, ZKGPU_CHECK_MAX_ROWS));
    }
    return s.tstop(timer);
}
int Checks::readback()
{
    uint64_t h[4 + ZKGPU_CHECK_MAX_ROWS];
    CK(zkgpu_memcpy_d2h(h, dev, sizeof h));
    res.n_bad = h[0];
    memcpy(res.rows, h + 1, ZKGPU_CHECK_MAX_ROWS * 8);
    for (int k = 0; k < 3; k++) res.value[k] = h[1 + ZKGPU_CHECK_MAX_ROWS + k] % P;
    res.ran = 1;
    pending = false;
    for (auto &v : names_ids) v.clear();
    for (auto &v : names_vals) v.clear();
    names_ran = names_on;
    if (names_on && res.n_bad) {
        // the names' block: only with a failing row, only its first min(n_bad, 16) rows count
        const size_t K = names_terms.size();
        std::vector<uint64_t> b(3 * K * ZKGPU_CHECK_MAX_ROWS);
        CK(zkgpu_memcpy_d2h(b.data(), names_dev, b.size() * 8));
        const uint64_t n_listed = std::min<uint64_t>(res.n_bad, ZKGPU_CHECK_MAX_ROWS);
        for (uint64_t j = 0; j < n_listed; j++)
            for (size_t k = 0; k < K; k++) {
                if (names_terms[k].dead) continue;
                uint64_t v[3];
                for (int t = 0; t < 3; t++) v[t] = b[(3 * k + t) * ZKGPU_CHECK_MAX_ROWS + j] % P;
                if (!(v[0] | v[1] | v[2])) continue;
                names_ids[j].push_back((uint32_t)k);
                names_vals[j].insert(names_vals[j].end(), v, v + 3);
            }
    }
    return 0;
}

// ---- naming (zkgpu_stark_check_names_set): which terms of C fail at the listed rows.
// zkgpu_zxp_split_constraints takes the n-domain step42ns apart once; the tapped program runs
// at the check's row list (zkgpu_zxp_eval_rows_dev) into a device block of 3K x 16 words of
// the names' own, outside the memory plan like the check's block.
int Checks::names_set(Starks &s, int on)
{
    names_on = false;
    std::string why;
    if (on && !names_prepare(s, why)) return fail("check_names_set: %s; naming is off", why.c_str());
    names_on = on != 0;
    return 0;
}
// the split of the n-domain step42ns (once) and the names' device block; false: `why` says
// what was refused (whether naming is on is the caller's business, as with prepare)
bool Checks::names_prepare(Starks &s, std::string &why)
{
    if (names_terms.empty()) {
        if (!prepare(s, why, false)) return false;
        const size_t ni = s.step42ns.instr.size(), no = s.step42ns.opnd.size();
        std::vector<zxp_instr> ti(2 * ni + 1);
        std::vector<zxp_operand> to(no + 2 * ni + 1);
        std::vector<zxp_split_term> tt(2 * ni + 1);
        uint32_t n_i = 0, n_o = 0, n_t = 0;
        if (zkgpu_zxp_split_constraints(ti.data(), &n_i, to.data(), &n_o, tt.data(), &n_t, s.step42ns.instr.data(),
                                        (uint32_t)ni, nd_opnd.data(), (uint32_t)no, 4)) {
            why = std::string("step42ns: ") + zkgpu_last_error();
            return false;
        }
        ti.resize(n_i), to.resize(n_o), tt.resize(n_t);
        names_instr.swap(ti), names_opnd.swap(to), names_terms.swap(tt);
    }
    if (!names_dev) {
        void *v = nullptr;
        if (zkgpu_dev_malloc(&v, 3 * names_terms.size() * ZKGPU_CHECK_MAX_ROWS * 8)) {
            why = zkgpu_last_error();
            return false;
        }
        names_dev = (uint64_t *)v;
    }
    return true;
}

// ---- a grand product that does not close: which values keep it open
// The failing path of z_all (a proof whose products close queues nothing
// of this): the multiset comparison (zkgpu_multiset_diff_dev) of the num
// and den tmpExp columns of the lowest open product, read back into
// zdiag before the failure returns.  For a permutation check (num = f +
// gamma, den = t + gamma) the lists are the offending values and where
// they first occur; the per-row factors of a plookup or connection
// product are not paired values: those faults are named by the audit's
// lookup misses and by conn_check / audit_conn below.
int Checks::z_open(Starks &s, uint32_t z, uint32_t n_open)
{
    zdiag = zkgpu_z_diag{};
    zdiag.z = z;
    zdiag.n_open = n_open;
    std::string why;
    if (!z_compare(s, z, zdiag.n_num, zdiag.n_den, zdiag.num, zdiag.den, why))
        return fail("calculateZ: grand product %u does not close (%u of %u do not); the comparison of its num and "
                    "den columns was skipped: %s", z, n_open, s.info.n_zctx, why.c_str());
    zdiag.ran = 1;
    char side[2][160];
    for (int b = 0; b < 2; b++) {
        const uint64_t cnt = b ? zdiag.n_den : zdiag.n_num;
        const zkgpu_z_diag_val &v = b ? zdiag.den[0] : zdiag.num[0];
        const char *name = b ? "den" : "num";
        if (cnt)
            snprintf(side[b], sizeof side[b], "%llu value(s) of %s unmatched, the first at row %llu (%llu in num, "
                     "%llu in den)", (unsigned long long)cnt, name, (unsigned long long)v.row,
                     (unsigned long long)v.count_num, (unsigned long long)v.count_den);
        else
            snprintf(side[b], sizeof side[b], "no value of %s unmatched", name);
    }
    return fail("calculateZ: grand product %u does not close (%u of %u do not): %s; %s", z, n_open, s.info.n_zctx,
                side[0], side[1]);
}

// the num and den columns of product z compared as multisets into the lists of zkgpu_z_diag (the
// audit's too); false: the scratch or the 98-word result block could not be had, `why` says which
bool Checks::z_compare(Starks &s, uint32_t z, uint64_t &n_num, uint64_t &n_den, zkgpu_z_diag_val *num,
                       zkgpu_z_diag_val *den, std::string &why)
{
    constexpr uint32_t M = ZKGPU_Z_DIAG_MAX, BLK = 1 + 3 * M;
    const uint64_t N = s.N;
    uint64_t h[2 * BLK];
    if (result_block(h, 2 * BLK, why, [&](uint64_t *dev) {
            return zkgpu_multiset_diff_dev(dev, s.S.sec[SEC_TMP_N] + (uint64_t)s.zctx[3 * z] * N, N,
                                           s.S.sec[SEC_TMP_N] + (uint64_t)s.zctx[3 * z + 1] * N, N, N, 3, M);
        }))
        return false;
    n_num = h[0];
    n_den = h[BLK];
    for (uint32_t k = 0; k < M; k++) {
        num[k] = {h[1 + 3 * k], h[2 + 3 * k], h[3 + 3 * k]};
        den[k] = {h[BLK + 1 + 3 * k], h[BLK + 2 + 3 * k], h[BLK + 3 + 3 * k]};
    }
    return true;
}

// ---- connection checks (include/zkgpu_stark.h zkgpu_stark_conn_set): conn_run names the cells
// that keep a declared product open (zkgpu_conn_breaks_dev over cm1_n and const_n, one
// synchronisation, a 99-word result block).  Neither section is written.
int Checks::conn_set(Starks &s, uint32_t z, const zkgpu_conn_desc *d)
{
    const zkgpu_stark_info &info = s.info;
    if (z >= info.n_zctx) return fail("conn_set: product %u: the instance has %u grand product(s)", z, info.n_zctx);
    if (!d) {
        conns.erase(z);
        return 0;
    }
    if (!d->cm1_cols || !d->const_cols) return fail("conn_set: product %u: null column list", z);
    if (zkgpu_conn_ks_check(d->ks, d->k, info.n_bits)) return fail("conn_set: product %u: %s", z, zkgpu_last_error());
    ConnDecl c;
    for (uint32_t i = 0; i < d->k; i++) {
        if (d->cm1_cols[i] >= info.n_cm1)
            return fail("conn_set: product %u: cm1 column %u: the instance has %u", z, d->cm1_cols[i], info.n_cm1);
        if (d->const_cols[i] >= info.n_const)
            return fail("conn_set: product %u: constant column %u: the instance has %u", z, d->const_cols[i],
                        info.n_const);
        for (uint32_t j = 0; j < i; j++)
            if (d->cm1_cols[j] == d->cm1_cols[i] || d->const_cols[j] == d->const_cols[i])
                return fail("conn_set: product %u: column %u repeated", z,
                            d->cm1_cols[j] == d->cm1_cols[i] ? d->cm1_cols[i] : d->const_cols[i]);
    }
    c.cm1_cols.assign(d->cm1_cols, d->cm1_cols + d->k);
    c.const_cols.assign(d->const_cols, d->const_cols + d->k);
    if (d->ks) c.ks.assign(d->ks, d->ks + d->k);
    conns[z] = std::move(c);
    return 0;
}

int Checks::conn_run(Starks &s, uint32_t z, const ConnDecl &c, zkgpu_conn_report &r, std::string &why)
{
    constexpr uint32_t M = ZKGPU_CONN_MAX;
    const uint64_t N = s.N;
    const uint32_t n_bits = s.info.n_bits;
    uint64_t h[3 + 6 * M];
    const int rc = result_block(h, 3 + 6 * M, why, [&](uint64_t *dev) {
        return zkgpu_conn_breaks_dev(dev, s.S.sec[SEC_CM1_N], N, c.cm1_cols.data(), s.S.sec[SEC_CONST_N], N,
                                     c.const_cols.data(), (uint32_t)c.cm1_cols.size(),
                                     c.ks.empty() ? nullptr : c.ks.data(), n_bits, M);
    });
    if (rc) return rc;
    r = zkgpu_conn_report{};
    r.ran = 1;
    r.z = z;
    r.n_broken = h[0], r.n_foreign = h[1], r.n_untargeted = h[2];
    for (uint32_t e = 0; e < M; e++) {
        const uint64_t *b = h + 3 + 4 * e, *f = h + 3 + 4 * M + 2 * e;
        zkgpu_conn_break &o = r.breaks[e];
        if (b[0] == UINT64_MAX)
            o = {UINT32_MAX, 0, UINT64_MAX, 0, 0, 0};
        else
            o = {(uint32_t)(b[0] >> n_bits), (uint32_t)(b[1] >> n_bits), b[0] & (N - 1), b[1] & (N - 1), b[2], b[3]};
        if (f[0] == UINT64_MAX)
            r.foreign[e] = {UINT32_MAX, UINT64_MAX, 0};
        else
            r.foreign[e] = {(uint32_t)(f[0] >> n_bits), f[0] & (N - 1), f[1]};
    }
    return 0;
}

int Checks::conn_check(Starks &s, uint32_t z, zkgpu_conn_report *out)
{
    if (!out) return fail("conn_check: null buffer");
    if (z >= s.info.n_zctx)
        return fail("conn_check: product %u: the instance has %u grand product(s)", z, s.info.n_zctx);
    const auto it = conns.find(z);
    if (it == conns.end()) return fail("conn_check: product %u is not declared a connection (conn_set)", z);
    if (s.need_trace("conn_check")) return -1;
    std::string why;
    if (conn_run(s, z, it->second, *out, why)) return fail("conn_check: product %u: %s", z, why.c_str());
    return 0;
}

// ---- trace audit (include/zkgpu_stark.h zkgpu_stark_audit): the stage-2
// and stage-3 work of prove_body on the n domain, run to the end whatever
// it finds, with challenges from a transcript that holds no root.  It
// writes tmpExp_n, cm2_n, cm3_n and the head of q -- every one dead between
// proofs under both plans -- and reads cm1_n, which it leaves as it is.
// The programs go through run(), not run_prog(): no probe record is taken.

// layer A's finding: the f values of plookup k that its table does not hold (a 34-word result block)
int Checks::audit_misses(Starks &s, uint32_t k, zkgpu_audit_pu &e)
{
    constexpr uint32_t M = ZKGPU_LOOKUP_MISS_MAX;
    const uint32_t *q = &s.pu[5 * k];
    const uint64_t N = s.N;
    uint64_t h[2 + 2 * M];
    std::string why;
    if (result_block(h, 2 + 2 * M, why, [&](uint64_t *dev) {
            return zkgpu_lookup_misses_dev(dev, s.S.sec[SEC_TMP_N] + (uint64_t)q[0] * N, N,
                                           s.S.sec[SEC_TMP_N] + (uint64_t)q[1] * N, N, N, q[4], M);
        }))
        return fail("audit: plookup %u: %s", k, why.c_str());
    e.pu = k;
    e.n_rows = h[0];
    e.n_vals = h[1];
    for (uint32_t j = 0; j < M; j++) e.vals[j] = {h[2 + 2 * j], h[3 + 2 * j]};
    return 0;
}

int Checks::audit(Starks &s, uint32_t flags, zkgpu_audit_report *out)
{
    if (!out) return fail("audit: null buffer");
    if (flags & ~ZKGPU_AUDIT_NAMES) return fail("audit: unknown flags 0x%x", flags);
    if (s.need_trace("audit")) return -1;
    audit_valid = false;
    audit_rep = zkgpu_audit_report{};
    for (zkgpu_conn_report &c : audit_conns) c = zkgpu_conn_report{};
    audit_why.clear();
    const auto tall = Starks::clk::now();
    // the audit's own challenges: verkey and publics, no root
    Transcript tr = s.begin_run(false);
    for (uint64_t &row : res.rows) row = UINT64_MAX;  // an empty list, should layer C not run
    zkgpu_audit_report &R = audit_rep;
    const uint64_t N = s.N;
    uint64_t ch[24] = {0};
    for (int k = 0; k < 4; k++) tr.get_field(ch + 3 * k);
    {
        Transcript fork = tr;  // (queue draws the same value from its own copy)
        uint64_t alpha[3];
        fork.get_field(alpha);
        if (fork.err) return fail("audit: transcript hashing failed: %s", zkgpu_last_error());
        memcpy(R.challenges, ch, 12 * 8);
        memcpy(R.challenges + 12, alpha, 24);
        memcpy(res.alpha, alpha, 24);  // (reported whether or not layer C runs)
    }
    const uint64_t ev0[3] = {0, 0, 0};
    // as a proof after stage 1: the columns no stage writes read 0
    if (s.lean() && (s.zero_unwritten(SEC_TMP_N) || s.zero_unwritten(SEC_CM2_N) || s.zero_unwritten(SEC_CM3_N)))
        return -1;
    // ---- layer A: every plookup
    if (s.timed("AUDIT_STEP2", [&] { return s.run(s.step2, false, ch, ev0, 0); })) return -1;
    if (s.info.n_pu) {
        s.tstart();
        for (uint32_t k = 0; k < s.info.n_pu; k++) {
            uint64_t miss = ~0ULL;
            if (!s.h1h2_one(k, miss)) continue;
            if (miss == ~0ULL) return fail("audit: calculateH1H2: %s", zkgpu_last_error());
            // a miss: h1 / h2 were not written; they read zero from here on
            const uint32_t *q = &s.pu[5 * k];
            CK(zkgpu_memset_dev(s.S.sec[SEC_CM2_N] + (uint64_t)q[2] * N, 0, (uint64_t)q[4] * N * 8));
            CK(zkgpu_memset_dev(s.S.sec[SEC_CM2_N] + (uint64_t)q[3] * N, 0, (uint64_t)q[4] * N * 8));
            if (R.n_pu_bad++ < ZKGPU_AUDIT_MAX_PU && audit_misses(s, k, R.pu[R.n_pu_bad - 1])) return -1;
        }
        if (s.tstop("AUDIT_H1H2")) return -1;
    }
    // ---- layer B: every grand product
    if (s.timed("AUDIT_STEP3PREV", [&] { return s.run(s.step3prev, false, ch, ev0, 0); })) return -1;
    s.tstart();
    {
        // (every z column is written, closed or not: layer C reads them)
        std::vector<int> closes;
        if (s.z_run(closes)) return -1;
        for (uint32_t z = 0; z < s.info.n_zctx; z++) {
            if (closes[z]) continue;
            if (R.n_z_open++ >= ZKGPU_AUDIT_MAX_Z) continue;
            zkgpu_audit_z &e = R.z[R.n_z_open - 1];
            e.z = z;
            // the products one after the other through the shared workspace; without the scratch
            // the product is still listed
            std::string why;
            e.compared = z_compare(s, z, e.n_num, e.n_den, e.num, e.den, why);
            // a declared connection: the cells that keep it open (ran = 0 without the scratch, as compared)
            const auto it = conns.find(z);
            if (it != conns.end()) (void)conn_run(s, z, it->second, audit_conns[R.n_z_open - 1], why);
        }
    }
    if (s.tstop("AUDIT_Z")) return -1;
    if (R.n_z_open) {  // zkgpu_stark_z_diag: the lowest open product
        const zkgpu_audit_z &e = R.z[0];
        zdiag.ran = e.compared;
        zdiag.z = e.z;
        zdiag.n_open = R.n_z_open;
        zdiag.n_num = e.n_num;
        zdiag.n_den = e.n_den;
        memcpy(zdiag.num, e.num, sizeof zdiag.num);
        memcpy(zdiag.den, e.den, sizeof zdiag.den);
    }
    // ---- layer C: the identities, unless a plookup missed (its h1 / h2 read zero)
    audit_named = false;
    audit_terms.clear();
    if (!R.n_pu_bad) {
        if (!s.step3.instr.empty() && s.timed("AUDIT_STEP3", [&] { return s.run(s.step3, false, ch, ev0, 0); }))
            return -1;
        if (prepare(s, audit_why)) {
            std::string why_names;
            const bool was_on = names_on;
            names_on = (flags & ZKGPU_AUDIT_NAMES) && names_prepare(s, why_names);  // refused: rows only
            const int rc = queue(s, tr, ch, "AUDIT_CONSTRAINTS") || readback();
            audit_named = names_on;
            if (audit_named) audit_terms.assign(names_ids, names_ids + ZKGPU_CHECK_MAX_ROWS);
            names_on = was_on;
            if (rc) return -1;
        }
    }
    R.identities = res;
    R.clean = !R.n_pu_bad && !R.n_z_open && res.ran && !res.n_bad;
    if (s.flush_timers()) return -1;
    if (tr.err) return fail("audit: transcript hashing failed: %s", zkgpu_last_error());
    s.timers.emplace_back("AUDIT_TOTAL", std::chrono::duration<double, std::milli>(Starks::clk::now() - tall).count());
    audit_valid = true;
    *out = R;
    return 0;
}

int Checks::audit_format(const Starks &s, char *buf, uint64_t len) const
{
    if (!audit_valid) return fail("audit_format: no audit has run on this prover");
    if (len && !buf) return fail("audit_format: null buffer");
    AuditContext c;
    c.n_bits = s.info.n_bits;
    c.n_pu = s.info.n_pu;
    c.n_zctx = s.info.n_zctx;
    c.identities_why = audit_why;
    c.named = audit_named;
    c.term_ids = audit_terms;
    c.conn.assign(audit_conns, audit_conns + ZKGPU_AUDIT_MAX_Z);
    const std::string text = zkgpu_host::audit_format(audit_rep, c);
    if (len) {
        const size_t n = std::min<size_t>(text.size(), len - 1);
        memcpy(buf, text.data(), n);
        buf[n] = 0;
    }
    return (int)text.size();
}

}  // namespace zkgpu_host
