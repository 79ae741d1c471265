// The proof schedule of the prover (starks.hpp): prove_body, the one
// Fiat-Shamir schedule of the single-GPU and the row-sharded prover, and its
// FRI and query part.
#include "starks.hpp"

namespace zkgpu_host {

// The one Fiat-Shamir schedule of the single-GPU and the row-sharded
// prover: the order of the transcript's inputs and challenges, the stage
// boundaries and the stage timers (the FRI part: fri_and_queries).  The
// row-sharded prover is never lean (shape() leaves mem_mode RESIDENT) and
// has neither a probe, a check nor streamed rows (its handle is refused at
// their entry points): those branches are dead there.
int Starks::prove_body(uint64_t *out)
{
    auto tall = clk::now();
    Transcript tr = begin_run(true);
    uint64_t ch[24] = {0};
    uint64_t roots[4][4];
    std::vector<uint64_t> evals(3 * info.n_ev);
    auto commit_root = [&](int t) {  // stage t's commit, its root into the transcript
        if (commit_stage(t, roots[t - 1])) return -1;
        tr.put(roots[t - 1], 4);
        return 0;
    };
    // STAGE 1 (starks.cpp:49-63)
    if (commit_root(1)) return -1;
    // lean: the regions of tmpExp_n / cm2_n / cm3_n held other sections;
    // the columns no stage writes read 0, as under the resident plan
    if (lean() && (zero_unwritten(SEC_TMP_N) || zero_unwritten(SEC_CM2_N) || zero_unwritten(SEC_CM3_N)))
        return -1;
    // probed: a column no stage of this proof has written yet reads 0 in a
    // record, as in a fresh prover (and the CPU provers' zeroed memory),
    // not the last proof's values or, lean, those of the region's former
    // section (the regions are dead here, as for zero_unwritten)
    if (probe.on())
        for (uint32_t s : {SEC_TMP_N, SEC_CM2_N, SEC_CM3_N})
            CK(zkgpu_memset_dev(S.sec[s], 0, (uint64_t)S.ncols[s] * N * 8));
    // STAGE 2 (:65-144)
    tr.get_field(ch + 0);
    tr.get_field(ch + 3);
    if (timed("STARK_STEP_2_CALCULATE_EXPS", [&] { return run_prog(ZKGPU_PROBE_STEP2, step2, ch, evals); })) return -1;
    if (info.n_pu && timed("STARK_STEP_2_CALCULATEH1H2", [&] {
            return probe.point(S, ZKGPU_PROBE_H1H2, 0, ch, evals) || h1h2_all() ||
                   probe.point(S, ZKGPU_PROBE_H1H2, 1, ch, evals);
        }))
        return -1;
    if (commit_root(2)) return -1;
    // STAGE 3 (:146-224)
    tr.get_field(ch + 6);
    tr.get_field(ch + 9);
    if (timed("STARK_STEP_3_CALCULATE_EXPS", [&] { return run_prog(ZKGPU_PROBE_STEP3PREV, step3prev, ch, evals); }))
        return -1;
    if (timed("STARK_STEP_3_CALCULATE_Z", [&] {
            return probe.point(S, ZKGPU_PROBE_Z, 0, ch, evals) || z_all() || probe.point(S, ZKGPU_PROBE_Z, 1, ch, evals);
        }))
        return -1;
    // step3: post-Z expressions (starks.cpp:193-208)
    if (!step3.instr.empty() &&
        timed("STARK_STEP_3_CALCULATE_EXPS_2", [&] { return run_prog(ZKGPU_PROBE_STEP3, step3, ch, evals); }))
        return -1;
    if (checks.run(*this, tr, ch)) return -1;  // the constraint check, where one is set
    if (commit_root(3)) return -1;
    // STAGE 4 (:226-296)
    tr.get_field(ch + 12);
    if (lean()) {
        // cm1_2ns again, over cm1_n (tmpExp_n / cm2_n above it are dead):
        // the columns not kept extended in place, the kept ones copied
        tstart();
        cm1_consumed = true;
        const uint64_t split = info.n_cm1 - keep_cols;
        if (split) CK(zkgpu_gl_extend_pol_inplace_dev(arena, NE, N, split));
        if (keep_cols) CK(zkgpu_memcpy_d2d(arena + split * NE, keep, keep_cols * NE * 8));
        S.sec[SEC_CM1_2NS] = arena;
        if (tstop("STARK_STEP_4_CM1_LDE")) return -1;
    }
    if (timed("STARK_STEP_4_CALCULATE_EXPS_2NS", [&] { return run_prog(ZKGPU_PROBE_STEP42NS, step42ns, ch, evals); }))
        return -1;
    if (timed("STARK_STEP_4_CALCULATE_EXPS_2NS_INTT_NTT", [&] {
            return probe.point(S, ZKGPU_PROBE_QSPLIT, 0, ch, evals) || quotient_pieces() ||
                   probe.point(S, ZKGPU_PROBE_QSPLIT, 1, ch, evals);
        }))
        return -1;
    if (commit_root(4)) return -1;
    // STAGE 5 (:298-392)
    tstart();
    uint64_t *xi = ch + 21;
    tr.get_field(xi);
    // Starks::evmap (starks.cpp:308-333,556-669) interpolates every
    // polynomial from its extension rows k << eb, the coset points
    // 7 w_N^k, with L = INTT((xi/7)^i).  The same values pol(xi) come
    // from the n-domain rows (points w_N^k) with L = INTT(xi^i): the
    // polynomial of degree < N is the same, the field sums are exact, and
    // contiguous n-domain columns read half the lines of the strided
    // extension rows.
    if (lean()) {
        // the extended rows k << eb are the points 7 w_N^k: the weights of
        // xi / 7 (starks.cpp:316-322)
        const uint64_t i7 = inv(7), xs[3] = {mul(xi[0], i7), mul(xi[1], i7), mul(xi[2], i7)};
        if (lagrange_xi(xs, r0(), nb)) return -1;
    } else if (lagrange_xi(xi, r0(), nb)) {
        return -1;
    }
    if (tstop("STARK_STEP_5_LEv_LpEv")) return -1;
    if (timed("STARK_STEP_5_EVMAP", [&] { return evmap_rows(r0(), nb, evals.data()) || sum_evals(evals); })) return -1;
    tr.put(evals.data(), evals.size());
    tr.get_field(ch + 15);
    tr.get_field(ch + 18);
    if (timed("STARK_STEP_5_XDIVXSUB", [&] { return xdivxsub(xi); })) return -1;
    if (timed("STARK_STEP_5_CALCULATE_EXPS",
              [&] { return run_prog(ZKGPU_PROBE_STEP52NS, step52ns, ch, evals) || fill_fri_pol0(); }))
        return -1;
    if (fri_and_queries(tr, &roots[0][0], evals, out, tall)) return -1;
    if (checks.finish()) return -1;
    return probe.readback(*this);
}

// FRIProve::prove + queries (friProve.cpp:5-232) once fri_pol[0] holds the
// FRI polynomial; s0 openings through open_s0
int Starks::fri_and_queries(Transcript &tr, const uint64_t *roots, const std::vector<uint64_t> &evals, uint64_t *out,
                            clk::time_point tall)
{
    tstart();
    uint64_t *w = out;
    memcpy(w, roots, 16 * 8);
    w += 16;
    memcpy(w, evals.data(), evals.size() * 8);
    w += evals.size();
    uint32_t pol_bits = info.n_bits_ext;
    uint64_t shift_inv = inv(7);
    int cur = 0;
    std::vector<uint64_t> fri_roots(4 * fri_steps.size(), 0);
    std::vector<uint64_t> final_pol(3ULL << fri_steps.back());
    for (size_t si = 0; si < fri_steps.size(); si++) {
        uint32_t red = pol_bits - fri_steps[si];
        uint64_t sx[3];
        tr.get_field(sx);
        if (si > 0) {
            if (fri_fold_step(si, fri_pol[cur ^ 1], fri_pol[cur], pol_bits, fri_steps[si], sx, shift_inv)) return -1;
            cur ^= 1;
        }
        if (si < fri_steps.size() - 1) {
            uint32_t nb = fri_steps[si + 1];
            uint64_t ngroups = 1ULL << nb;
            uint64_t width = (3ULL << fri_steps[si]) / ngroups;
            // (layer 0 of a prover that keeps f in row blocks: no whole
            // fri_pol[0] exists, the override reads the blocks)
            const uint64_t *pol = si == 0 && !fri_pol0_filled() ? nullptr : fri_pol[cur];
            if (fri_transpose_layer(si, fri_aux[si + 1], pol, 1ULL << fri_steps[si], nb)) return -1;
            if (fri_commit(si + 1, ngroups, width, &fri_roots[4 * (si + 1)])) return -1;
            tr.put(&fri_roots[4 * (si + 1)], 4);
        } else {
            CK(zkgpu_memcpy_d2h(final_pol.data(), fri_pol[cur], final_pol.size() * 8));
            tr.put(final_pol.data(), final_pol.size());
        }
        pol_bits = fri_steps[si];
        for (uint32_t j = 0; j < red; j++) shift_inv = mul(shift_inv, shift_inv);
    }
    if (tstop("STARK_STEP_FRI_FOLDS")) return -1;
    tstart();
    std::vector<uint64_t> ys(q());
    tr.get_permutations(ys.data(), q(), fri_steps[0]);
    pend.clear();
    pend_idx.clear();
    // FRI layers si >= 1: root, vals, siblings
    std::vector<uint64_t> yq = ys;
    for (size_t si = 0; si < fri_steps.size(); si++) {
        if (si > 0) {  // root, then the openings written in place (at flush_opens at the latest)
            uint64_t ngroups = 1ULL << fri_steps[si];
            uint64_t width = (3ULL << fri_steps[si - 1]) / ngroups;
            memcpy(w, &fri_roots[4 * si], 32);
            w += 4;
            uint64_t *vals = w, *sibs = w + q() * width;
            w = sibs + (uint64_t)q() * fri_steps[si] * 4;
            if (fri_open(si, ngroups, width, yq, vals, sibs)) return -1;
        }
        if (si < fri_steps.size() - 1)
            for (auto &y : yq) y %= (1ULL << fri_steps[si + 1]);
    }
    if (open_s0(ys, w) || flush_opens()) return -1;
    memcpy(w, final_pol.data(), final_pol.size() * 8);
    w += final_pol.size();
    if (tstop("STARK_STEP_FRI_QUERIES") || flush_timers()) return -1;
    if (tr.err) return fail("transcript hashing failed: %s", zkgpu_last_error());
    if ((uint64_t)(w - out) != proof_len()) return fail("proof length mismatch");
    timers.emplace_back("STARK_TOTAL", std::chrono::duration<double, std::milli>(clk::now() - tall).count());
    if (exec_commit_ms >= 0) {  // the hand-off that loaded this proof's trace (set_cm1_witness), outside the total
        timers.emplace_back("ZKGPU_EXEC_COMMIT", exec_commit_ms);
        exec_commit_ms = -1.0;
    }
    return 0;
}

}  // namespace zkgpu_host
