/*
 * zkgpu_stark.h -- C-ABI of libzkgpu_stark, the host-side STARK prover
 * (a C++ restatement of Starks::genProof, starks.cpp:9-404, and
 * FRIProve::prove, friProve.cpp:5-190) that drives the MI355X kernels only
 * through include/zkgpu.h.  The instance description plays the role of the
 * reference's StarkInfo (stark_info.hpp:269-336) + Steps (steps.hpp).
 *
 * Proof output: one flat u64 buffer in the reference's zkin order
 * (proof2zkinStark.cpp:8-82), canonical values:
 *   root1[4] root2[4] root3[4] root4[4] evals[n_ev*3]
 *   for si = 1 .. n_fri_steps-1:
 *       s{si}_root[4]  s{si}_vals[Q][3*2^(steps[si-1]-steps[si])]  s{si}_siblings[Q][steps[si]][4]
 *   s0_vals1[Q][n_cm1] s0_vals2[Q][n_cm2] s0_vals3[Q][n_cm3] s0_vals4[Q][n_cm4] s0_valsC[Q][n_const]
 *   s0_siblings{1,2,3,4,C}[Q][n_bits_ext][4]
 *   finalPol[2^steps[last]][3]
 */
#ifndef ZKGPU_STARK_H
#define ZKGPU_STARK_H
#include <stdint.h>

#include "zkgpu_zxp.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    const zxp_instr *instr;
    uint32_t n_instr;
    const zxp_operand *opnd;
    uint32_t n_opnd;
    uint32_t n_tmp1, n_tmp3;
} zkgpu_zxp_prog;

typedef struct {
    uint32_t n_bits, n_bits_ext, n_queries, n_fri_steps;
    uint32_t fri_steps[32];
    uint32_t n_cm1, n_cm2, n_cm3, n_cm4, n_tmp, n_const, n_publics, q_deg, l_first, n_k;
    uint64_t seed;
    uint32_t n_random_cols;
    const uint32_t *random_cols; /* cm1 columns filled by the trace generator */
    uint32_t n_zctx;
    const uint32_t *zctx; /* (num tmp col, den tmp col, z cm3 col) triples */
    uint32_t n_ev;
    const uint32_t *ev; /* evMap (section_2ns, col, dim, prime) quads */
    zkgpu_zxp_prog step1, step2, step3prev, step42ns, step52ns;
    /* constant polynomials (setup; the reference loads them from the
     * zkevmConstPols file, starks.hpp:94-116): these columns are filled
     * pseudo-randomly (n_random_const = 0: columns 0 .. n_k-1), l_first gets
     * L_first, then step0 derives the rest on the N domain (may be empty) */
    uint32_t n_random_const;
    const uint32_t *random_const;
    zkgpu_zxp_prog step0;
    /* plookups (starkInfo.puCtx, starks.cpp:104-127): (f tmp col, t tmp col,
     * h1 cm2 col, h2 cm2 col, dim) quintuples; h1/h2 are computed after step2 */
    uint32_t n_pu;
    const uint32_t *pu;
    /* post-Z stage-3 expressions (starks.cpp:193-208, Steps::step3_parser_first):
     * run after calculateZ, before the stage-3 LDE + commit (may be empty) */
    zkgpu_zxp_prog step3;
} zkgpu_stark_info;

/* allocate the HBM memory map, build the constant polynomials, their LDE and
 * the constant tree (the reference loads these from files; setup, untimed).
 * Memory plan ZKGPU_MEM_AUTO (below). */
int zkgpu_stark_create(void **handle, const zkgpu_stark_info *info);

/* HBM plans of the single-GPU prover (the reference allocates one memory map
 * for the prover's life and reuses sections as scratch, prover.cpp:94,
 * starks.cpp:53,105):
 *   RESIDENT  every section of both domains held for the prover's life: the
 *             trace survives a proof (prove may run again on it).
 *   LEAN      one arena whose regions follow the sections' lifetimes within a
 *             proof: cm1's stage-1 extension is hashed and dropped, the
 *             n-domain sections die after stage 3, cm3 and (before stage 4)
 *             cm1 are extended in place over their n-domain values, evmap
 *             reads the extended rows k << blowup (starks.cpp:308-333).  The
 *             proof consumes cm1_n: set_cm1 / witness before every prove
 *             (prove fails loudly otherwise); set_cm1_async is not offered.
 *             At the fork-9 widths and 2^23 rows: about 260 GB instead of 386.
 *   AUTO      RESIDENT when its plan fits the device's free HBM, else LEAN.
 * Proofs are bit-identical under every plan. */
enum { ZKGPU_MEM_AUTO = 0, ZKGPU_MEM_RESIDENT = 1, ZKGPU_MEM_LEAN = 2 };
int zkgpu_stark_create_ex(void **handle, const zkgpu_stark_info *info, uint32_t memory_plan);
/* the plan a single-GPU prover runs under (ZKGPU_MEM_RESIDENT / _LEAN) */
int zkgpu_stark_memory_mode(void *handle);
/* synthetic committed trace cm1_n (executor stand-in: PRNG columns + step1) */
int zkgpu_stark_witness(void *handle);
/* load cm1_n from a host row-major buffer (n rows x n_cm1), the reference's
 * commit-pols layout (commit_pols.hpp:18) */
int zkgpu_stark_set_cm1(void *handle, const uint64_t *rows);
/* queue the trace of the proof AFTER the next one: returns at once, the
 * trace crosses PCIe into a second cm1_n buffer (zkgpu_load_rows_async)
 * while the next zkgpu_stark_prove runs on the current cm1_n, and becomes
 * cm1_n when that prove returns.  `rows` must stay valid until then; a later
 * set_cm1 / set_cm1_async supersedes it.  Costs one more cm1_n (n x n_cm1
 * u64; a shard's rows on a sharded prover) of HBM.  On a sharded prover each
 * rank passes the whole row-major buffer and loads its own rows, as with
 * set_cm1. */
int zkgpu_stark_set_cm1_async(void *handle, const uint64_t *rows);
/* The recursion STARKs' way in (C12a, recursive1, recursive2, recursiveF: prover.cpp:591-593,
 * 629-630, Circom*::getCommitedPols): the committed trace comes from a circom witness through the
 * circuit's .exec file, on the GPU (zkgpu_exec_*, include/zkgpu.h) -- size_witness words cross
 * PCIe instead of n x n_cm1.
 * set_exec: once per circuit; image / image_words are the .exec file's u64 words, planned for
 *   n_cm1 columns.  Refused with the planner's message (which names the add or cell), and when the
 *   sMap has more than n rows.  The plan's tables and its tmp buffer are one device block outside
 *   the memory plan (zkgpu_exec_info's device_bytes: 28 bytes an add, 4 a cell, 8 a slot); failing
 *   to allocate it is an error.  A later set_exec replaces the plan.
 * set_cm1_witness: witness (host, size_witness words, free again on return) -> cm1_n.  Leaves the
 *   prover exactly as set_cm1 of the reference's buffer would, under either memory plan: prove,
 *   audit and the constraint check may follow, a pending set_cm1_async load is superseded.  Its
 *   wall time is the timer ZKGPU_EXEC_COMMIT: alone in zkgpu_stark_timers until the next proof,
 *   then the last line of that proof's timers (outside STARK_TOTAL).
 * Both are refused on a sharded handle; set_cm1_witness before set_exec. */
int zkgpu_stark_set_exec(void *handle, const uint64_t *image, uint64_t image_words, uint64_t size_witness);
int zkgpu_stark_set_cm1_witness(void *handle, const uint64_t *witness);
/* cm1_n back into a host row-major buffer (n rows x n_cm1; the inverse of
 * set_cm1).  Single-GPU prover only. */
int zkgpu_stark_get_cm1(void *handle, uint64_t *rows);
/* load the constant polynomials from a host row-major buffer (n rows x
 * n_const), the reference's .const file (ConstantPolsStarks, starks.hpp:94-116);
 * recomputes their LDE, tree and verkey */
int zkgpu_stark_set_const(void *handle, const uint64_t *rows);
/* set the public inputs (n_publics values; prover.cpp:480-560 computes them
 * from the executor's Main columns) */
int zkgpu_stark_set_publics(void *handle, const uint64_t *publics);
uint64_t zkgpu_stark_proof_len(void *handle);
int zkgpu_stark_prove(void *handle, uint64_t *proof_out);
/* One proof of the executor's host buffer (n rows x n_cm1, row-major): the
 * trace is loaded in column batches while stage 1 extends and hashes the
 * batches already on the device.  Same proof as set_cm1(rows) + prove().
 * Where the reference starts (prover.cpp:94-116,435: genProof on cmPols in
 * host memory).  Offered under both single-GPU plans -- the lean plan's way
 * to overlap the upload, where set_cm1_async is refused -- not on a sharded
 * prover.  register_host = 1 page-locks `rows` for the call; a pinned or
 * registered source is what overlaps (a pageable one stays correct, its
 * copies block the calling thread).  Batches are 128 columns, 64 for a trace
 * narrower than 256 (ZKGPU_STREAM_COLS overrides, tests); stage 1 is reported as one timer,
 * STARK_STEP_1_STREAM.  Afterwards as after set_cm1 + prove: the trace is
 * consumed under LEAN, get_cm1 returns `rows` under RESIDENT.  A pending
 * set_cm1_async load is dropped.  If a load fails mid-stream the call fails
 * with the loader's message once everything queued has drained, and prove /
 * get_cm1 are refused until set_cm1 / witness / a successful
 * prove_from_rows loads a whole trace. */
int zkgpu_stark_prove_from_rows(void *handle, const uint64_t *rows, int register_host, uint64_t *proof_out);
int zkgpu_stark_verkey(void *handle, uint64_t out[4]);
int zkgpu_stark_publics(void *handle, uint64_t *out);
/* STARK_STEP_* timers of the last prove (starks.cpp:49-403 names):
 * names '\n'-separated into names_buf, milliseconds into ms; returns count */
int zkgpu_stark_timers(void *handle, char *names_buf, uint64_t names_len, double *ms, uint32_t max);
void zkgpu_stark_destroy(void *handle);
const char *zkgpu_stark_last_error(void);

/* ---- probe: sampled rows around every stage program of a proof ------------
 * At the full size the sections are tens of GB and live for a fraction of a
 * second, so the columns the prover computes on the way (tmpExp, cm2, cm3,
 * q, cm4, f) can only be looked at as a sample of rows taken at the moment
 * each program runs.  The caller names rows of the n and of the extended
 * domain; during every later proof the prover records, at each point below,
 * those rows (plus the rows the point's shifted accesses reach) of every
 * section the point's program reads (before it runs) and stores to (after),
 * from the section table in force at that moment, with the challenges and
 * evaluations in force.  A checker re-evaluates the source program on those
 * rows (tests/zxp_rows.py); against another prover the first differing record
 * names the first differing stage.
 *
 * Records, in order, per point:
 *   1 SCALARS record (after = 0, one "row" 0, ncols = 24 + 3 n_ev):
 *     challenges[24] (those not drawn yet read 0), then evals[3 n_ev] (zero
 *     before stage 5);
 *   program points (STEP2, STEP3PREV, STEP3 -- only when the instance has
 *   that program --, STEP42NS, STEP52NS): after = 0 records of the sections
 *   the program reads, ascending, then after = 1 records of the sections it
 *   stores to, ascending.  Rows of a section: the ascending union of
 *   (r + s) mod dom over the sampled rows r of the program's domain and s in
 *   {0} + every row shift the program uses with that section (reads and
 *   stores).  An empty program has the SCALARS record only;
 *   H1H2 (only with plookups): after = 1, SEC_CM2_N; Z: after = 1, SEC_CM3_N;
 *   QSPLIT: after = 1, SEC_CM4_2NS -- on the sampled rows of their domain.
 * Every record covers its section's whole width.  Each record is one
 * zkgpu_gather_rows_dev on the prover's stream into a device block allocated
 * by probe_set (outside the memory plan); no host synchronisation is added
 * inside the proof, one device-to-host copy follows it (timer line
 * ZKGPU_PROBE_READBACK, after STARK_TOTAL).  A probed proof also zeroes
 * tmpExp_n / cm2_n / cm3_n after stage 1, so that a column no stage has written
 * yet reads 0 in a record (not an earlier proof's values, or under the lean
 * plan the region's former section's).  With no probe set a proof launches
 * exactly what it launched before. */
enum { ZKGPU_PROBE_STEP2 = 0, ZKGPU_PROBE_H1H2, ZKGPU_PROBE_STEP3PREV, ZKGPU_PROBE_Z, ZKGPU_PROBE_STEP3,
       ZKGPU_PROBE_STEP42NS, ZKGPU_PROBE_QSPLIT, ZKGPU_PROBE_STEP52NS, ZKGPU_PROBE_POINTS };
#define ZKGPU_PROBE_SCALARS 0xFFFFFFFFu   /* record "section": challenges[24] then evals[3 * n_ev] */
#define ZKGPU_PROBE_MAX_ROWS 4096u

typedef struct {
    uint32_t point;    /* ZKGPU_PROBE_* */
    uint32_t after;    /* 0: taken before the point ran, 1: after */
    uint32_t section;  /* SEC_* or ZKGPU_PROBE_SCALARS */
    uint32_t ncols;    /* the section's whole width */
    uint64_t n_rows;
    uint64_t rows_off; /* into the u64 payload: n_rows row indices, strictly ascending */
    uint64_t vals_off; /* into the u64 payload: n_rows x ncols, row-major */
} zkgpu_probe_rec;

/* rows_n / rows_ext: sampled rows of the n and the extended domain (each <= ZKGPU_PROBE_MAX_ROWS,
 * in range, repeats folded); both empty: probe off.  Holds for every later proof until changed.
 * Refused: a sharded prover, a row out of range, too many rows, a program that reads or writes
 * a section of the other domain than its own.  A refusal or a failed allocation leaves the probe off. */
int zkgpu_stark_probe_set(void *handle, const uint64_t *rows_n, uint32_t n_rows_n,
                          const uint64_t *rows_ext, uint32_t n_rows_ext);
/* record count and payload length (u64) of the last successful proof's probe; 0/0 when there is none */
int zkgpu_stark_probe_size(void *handle, uint32_t *n_recs, uint64_t *n_words);
int zkgpu_stark_probe_read(void *handle, zkgpu_probe_rec *recs, uint32_t max_recs, uint64_t *payload, uint64_t max_words);

/* ---- constraint check: the trace rows that break the AIR, before stage 4 ------
 * A trace row that breaks a polynomial identity goes through a proof silently:
 * stage 4 divides whatever step42ns computes by Z_H on the coset and the proof
 * that comes out verifies nowhere.  With the check on, prove / prove_from_rows
 * evaluate, between the last stage-3 program and stage 3's commit, the
 * constraint combination C that step42ns forms before its final "x ZI" on the
 * n domain itself (the program rewritten once by zkgpu_zxp_to_n_domain,
 * include/zkgpu.h; its output borrows the head of q, nothing is added to a
 * memory plan), and reduce it to the rows where C != 0
 * (zkgpu_nonzero_rows_dev).  C vanishes on every row iff every identity holds
 * there, with overwhelming probability over the combination challenge.  The
 * check itself names ROWS; zkgpu_stark_check_names_set (below) adds the
 * constraints that fail at them.
 *
 * The combination challenge: the transcript's challenge 4 is drawn from root 3,
 * which does not exist yet, so the check uses the getField of a COPY of the
 * transcript taken after challenges 2 and 3 (returned in `alpha`); the proof's
 * transcript is untouched and a checked proof is the unchecked one bit for bit.
 *
 *   OFF     a proof queues exactly what it queued before.
 *   REPORT  no host synchronisation is added inside the proof; the result is
 *           read back after it, and prove returns what it would have returned.
 *   STOP    one synchronisation at the check; with n_bad > 0 prove fails there
 *           with a message naming the domain size, n_bad and the first failing
 *           row, nothing of stage 3's commit or later is queued, and the prover
 *           is left as after any other failed proof (under the lean plan the
 *           trace has not been consumed).
 * Timer line ZKGPU_CHECK_CONSTRAINTS, present only when the check ran.
 * check_set rewrites the instance's step42ns once; a program the rewrite refuses
 * makes it fail with that message and leaves the check off.  Refused: a sharded
 * prover, an unknown mode.  Holds for every later proof until changed. */
enum { ZKGPU_CHECK_OFF = 0, ZKGPU_CHECK_REPORT = 1, ZKGPU_CHECK_STOP = 2 };
#define ZKGPU_CHECK_MAX_ROWS 16
typedef struct {
    uint32_t ran;                         /* 1: the last prove reached the check */
    uint64_t n_bad;                       /* rows of the n domain where C != 0 */
    uint64_t rows[ZKGPU_CHECK_MAX_ROWS];  /* the lowest of them, ascending; UINT64_MAX past the last */
    uint64_t value[3];                    /* C at rows[0], canonical (0 when n_bad = 0) */
    uint64_t alpha[3];                    /* the combination challenge used (above) */
} zkgpu_check_result;
int zkgpu_stark_check_set(void *handle, uint32_t mode);
int zkgpu_stark_check_result(void *handle, zkgpu_check_result *out);

/* Naming: which identities fail at the listed rows.  step42ns folds its identities into C with
 * powers of the combination challenge; zkgpu_zxp_split_constraints (include/zkgpu.h) takes that
 * combination apart into terms -- the k-th term is the k-th identity folded, in the producer's
 * (pil-stark's) order, and terms[k].instr is the step42ns instruction at which it joined -- and
 * with naming on a checked proof also evaluates every term at the check's listed rows: ONE more
 * launch (zkgpu_zxp_eval_rows_dev, kernel k_zxp_eval_rows, whose waves return at once when no row
 * is listed) behind the check's, into a device block of 3 x n_terms x 16 words allocated by
 * names_set outside the memory plan.  REPORT still adds no synchronisation inside the proof; the
 * block is read back with the check's result, and only when n_bad > 0.  The row result
 * (zkgpu_check_result) is unchanged, and with naming off a checked proof queues what it queued
 * before.  STOP's failure message gains a tail naming up to 8 failing terms at the first row.
 *   names_set    on != 0: splits the n-domain step42ns once; a program the split refuses makes it fail
 *                with that message and leaves naming off (the row check is unaffected).  Refused:
 *                a sharded prover.  Holds for every later checked proof until changed.
 *   check_terms  the term table: *n = n_terms, min(max, n_terms) entries written.
 *   check_named  for the failing row rows[slot] (slot < 16) of the last checked proof: *n_failing =
 *                the number of live terms that are not zero there, and the first min(max, that)
 *                of them: ids ascending, values canonical (3 words each).  C at that row is the
 *                sum of (-1)^negated * alpha^exponent * value over them.  A slot past the last
 *                failing row is empty.  Fails when the last proof ran no check with naming on. */
int zkgpu_stark_check_names_set(void *handle, int on);
int zkgpu_stark_check_terms(void *handle, zxp_split_term *out, uint32_t max, uint32_t *n);
int zkgpu_stark_check_named(void *handle, uint32_t slot, uint32_t *ids, uint64_t *values, uint32_t max,
                            uint32_t *n_failing);

/* ---- a grand product that does not close: the values that keep it open
 * calculateZ (starks.cpp:165-189) of a product whose total is not 1 fails the proof with
 * "calculateZ: grand product <z> does not close".  Before that failure returns, the single-GPU
 * prover compares the num and den tmpExp columns (dim 3) of the LOWEST such product as multisets
 * (zkgpu_multiset_diff_dev, include/zkgpu.h, 16 values per side), reads the result back and
 * keeps it; the message gains a tail naming, per side, how many distinct values are unmatched,
 * the first one's row and its two counts.  The return code and the state the failed proof leaves
 * are unchanged.
 *   num[k] / den[k]  the k-th value, by its first row on that side, whose count in num differs
 *                    from its count in den: {that row, count in num, count in den};
 *                    {UINT64_MAX, 0, 0} past the last.  n_num / n_den count all of them.
 * What the lists mean: for a permutation check (num = f + gamma, den = t + gamma) they are
 * exactly the offending values and where they first occur -- a tuple on one side only, or a
 * default value with one copy too many ("5000001 times against 5000000").  The per-row factors of
 * a plookup or a connection product are not paired values, so there the lists do not name the
 * fault: a plookup's missing values come from zkgpu_lookup_misses_dev (layer A of the audit
 * below), a connection's unequal cells from zkgpu_stark_conn_check / zkgpu_stark_audit_conn
 * (below).
 * A proof whose products all close queues nothing of this: no kernel, no allocation, the same
 * timers, the same proof; nothing is added to either memory plan's figure (the comparison's
 * scratch is the library workspace, zkgpu_multiset_diff_workspace_bytes(n), taken on the failing
 * path only).  When that scratch cannot be allocated the message says the comparison was skipped
 * and ran stays 0.  The row-sharded prover keeps the plain message; zkgpu_stark_z_diag on its
 * handle is refused (single-GPU provers only, as the constraint check). */
#define ZKGPU_Z_DIAG_MAX 16
typedef struct { uint64_t row, count_num, count_den; } zkgpu_z_diag_val;
typedef struct {
    uint32_t ran;       /* 1: the last prove failed at calculateZ and the comparison ran */
    uint32_t z;         /* the lowest product that does not close (index into zctx) */
    uint32_t n_open;    /* how many products do not close */
    uint64_t n_num, n_den;                       /* distinct values with unequal counts, by side */
    zkgpu_z_diag_val num[ZKGPU_Z_DIAG_MAX], den[ZKGPU_Z_DIAG_MAX];
} zkgpu_z_diag;
int zkgpu_stark_z_diag(void *handle, zkgpu_z_diag *out);

/* ---- trace audit: every broken plookup, product and identity of a loaded trace, no proof
 * The diagnoses above run inside a proof and end it at the first finding: stage 1's LDE and tree
 * come first, the first plookup with a miss or the lowest open product is the last thing the
 * proof says.  The audit runs the stage-2 and stage-3 work of a proof on the n domain and nothing
 * else -- no LDE, no tree, no stage 4 or 5, no FRI, nothing committed -- to the end, and reports
 * everything it finds in one call.
 *
 * NOT A VERIFIER.  With no roots to draw from, the audit's challenges come from a transcript that
 * holds the verkey and the publics only: ch0 .. ch3 are its first four getField, the combination
 * challenge the fifth.  They are not the proof's challenges and do not depend on the trace, so a
 * trace built on purpose could be fitted to them: the audit is an aid against executor bugs, not
 * a soundness check.  Rows, counts, first rows and term ids do not depend on the challenges (with
 * overwhelming probability); the values at the failing rows do.
 *
 *   A  plookups, every one of n_pu: step2, then calculateH1H2 per plookup.  Where it reports a
 *      miss the plookup's h1 / h2 columns of cm2_n are zeroed, zkgpu_lookup_misses_dev
 *      (include/zkgpu.h) lists the f values its table does not hold, and the audit goes on to the
 *      next plookup.  The lowest ZKGPU_AUDIT_MAX_PU failing plookups are detailed, all are counted.
 *   B  grand products, every one of n_zctx: step3prev, then calculateZ (which writes every z
 *      column whether or not its product closes).  Each of the lowest ZKGPU_AUDIT_MAX_Z open
 *      products has its num and den columns compared as multisets (zkgpu_multiset_diff_dev, the
 *      lists of zkgpu_z_diag; compared = 0 when the scratch could not be allocated: the product is
 *      still listed).  A plookup that missed leaves its own product open (its h1 / h2 read zero):
 *      that entry follows from layer A's and says nothing new.
 *   C  identities: the post-Z step3 program, then the constraint combination on the n domain with
 *      the audit's challenge (the constraint check above; the first use rewrites step42ns as
 *      check_set does), with ZKGPU_AUDIT_NAMES also the terms at the failing rows (as
 *      check_names_set; a combination the split refuses degrades to rows only).  An open product
 *      does not stop it: its boundary identity fails on a row or two and the names say which.  A
 *      plookup that missed does: h1 / h2 are meaningless and C would fail on almost every row --
 *      identities.ran = 0 then, as for a step42ns the n-domain rewrite refuses (layers A and B
 *      still run; zkgpu_stark_audit_format says which it was).
 *
 * A dirty trace is not a failed call: audit returns 0 whenever it ran to the end and `clean`
 * carries the verdict.  Refused, with a message: a sharded handle (single-GPU provers only), no
 * whole trace loaded (before any set_cm1 / witness, after a failed streamed load, under the lean
 * plan after a proof consumed the trace).
 * Afterwards: the trace is untouched and not consumed under either plan -- prove() may follow
 * directly and gives the proof it would have given; a pending set_cm1_async load is left alone; no
 * probe records are taken; check_set's mode and check_names_set's are neither consulted nor
 * changed.  zkgpu_stark_check_result / check_terms / check_named and zkgpu_stark_z_diag (the lowest
 * open product, or ran = 0) refer to the audit as the latest run; zkgpu_stark_timers gives AUDIT_*
 * lines (AUDIT_STEP2, AUDIT_H1H2, AUDIT_STEP3PREV, AUDIT_Z, AUDIT_STEP3, AUDIT_CONSTRAINTS,
 * AUDIT_TOTAL).  One synchronisation per layer.  Nothing is added to a memory plan: the scratch
 * is the library workspace and result blocks allocated when a finding needs them. */
#define ZKGPU_AUDIT_NAMES 1u      /* flags: also evaluate the terms of the combination at the failing rows */
#define ZKGPU_AUDIT_MAX_PU 8
#define ZKGPU_AUDIT_MAX_Z 8
#define ZKGPU_LOOKUP_MISS_MAX 16
typedef struct { uint64_t row, count; } zkgpu_lookup_miss;
typedef struct {
    uint32_t pu;              /* index into pu */
    uint64_t n_rows, n_vals;  /* rows of f whose value the table does not hold; distinct such values */
    zkgpu_lookup_miss vals[ZKGPU_LOOKUP_MISS_MAX]; /* {first row in f, rows in f}, by row; {UINT64_MAX, 0} past the last */
} zkgpu_audit_pu;
typedef struct {
    uint32_t z, compared;     /* index into zctx; 1: the lists below are filled */
    uint64_t n_num, n_den;
    zkgpu_z_diag_val num[ZKGPU_Z_DIAG_MAX], den[ZKGPU_Z_DIAG_MAX];
} zkgpu_audit_z;
typedef struct {
    uint32_t clean;                 /* 1: no layer found anything */
    uint64_t challenges[15];        /* the audit's own: ch0..ch3 and the combination challenge */
    uint32_t n_pu_bad;  zkgpu_audit_pu pu[ZKGPU_AUDIT_MAX_PU];   /* the lowest failing plookups */
    uint32_t n_z_open;  zkgpu_audit_z  z[ZKGPU_AUDIT_MAX_Z];     /* the lowest open products */
    zkgpu_check_result identities;  /* ran = 0 when a plookup missed (above) */
} zkgpu_audit_report;
int zkgpu_stark_audit(void *handle, uint32_t flags, zkgpu_audit_report *out);
/* the report of the last audit as text, one finding per line in the wording of the proof's failure
 * messages; returns the length the whole text needs (without the terminator), at most len - 1
 * characters are written; fails when no audit has run on the handle */
int zkgpu_stark_audit_format(void *handle, char *buf, uint64_t len);

/* ---- connection checks: the cells a copy constraint leaves unequal
 * A plonk-style circuit (C12a, recursive1, recursive2) asserts nearly everything about its
 * witness through one connection check {a[0..k-1]} connect {S[0..k-1]} (the starkinfo's ciCtx):
 * cell (i, r) of committed column a_i must hold the value of the cell that the constant column
 * S_i names at row r (include/zkgpu.h zkgpu_conn_breaks_dev: identities, coset shifts ks and
 * what broken, foreign and untargeted mean).  When its grand product does not close, what a
 * developer needs is which two wired cells differ; the product's num / den lists cannot say.
 *   conn_set    declares product z of zctx as the connection of the k cm1 columns cm1_cols with
 *               the k constant columns const_cols (the starkinfo carries expression ids only, so
 *               the caller tells them) and the shifts ks (NULL: 12^i, pil-stark's getKs with
 *               k = 12 -- an assumption, see zkgpu_conn_breaks_dev).  The description is copied;
 *               d = NULL clears the declaration.  Refused: z >= n_zctx, a column past n_cm1 /
 *               n_const or repeated, k = 0 or > 64, ks with a zero or colliding cosets.
 *   conn_check  runs the primitive over cm1_n and const_n of the loaded trace and returns the
 *               report: no stage program, no challenge, one synchronisation; the trace is not
 *               touched and nothing is added to either memory plan (the scratch is the library
 *               workspace, zkgpu_conn_breaks_workspace_bytes(n, k)).  Needs a whole trace
 *               loaded, as the audit; refused for an undeclared product.
 *   audit       (zkgpu_stark_audit, layer B) for each LISTED open product with a declared
 *               connection the same routine runs and its report is kept; a closed product queues
 *               nothing, and a prover with no declaration audits exactly as before.  The
 *               zkgpu_audit_report keeps its layout: audit_conn(k) returns the report that goes
 *               with report.z[k] of the last audit, ran = 0 when that entry is no declared
 *               connection, is not listed, or the scratch could not be had.
 * In a report col / to_col are indices into the declaration's column lists (pols[i]), rows are
 * trace rows, values canonical.  breaks holds the lowest ZKGPU_CONN_MAX broken cells by (col,
 * row), {UINT32_MAX, 0, UINT64_MAX, 0, 0, 0} past the last; foreign likewise, {UINT32_MAX,
 * UINT64_MAX, 0} past the last.  One wrong cell inside a cycle is two entries, both naming it.
 * zkgpu_stark_audit_format prints, under the product's calculateZ line,
 *   "  connection: 2 cell(s) differ from the cell they are wired to; pols[1] row 37 (= 5) is
 *    wired to pols[0] row 28 (= 6)", one line per listed break, "and N more", and the foreign
 * and untargeted counts when they are not zero.
 * The proving path (prove's own calculateZ failure) is unchanged.  Single-GPU provers only. */
typedef struct { uint32_t k; const uint32_t *cm1_cols, *const_cols; const uint64_t *ks; } zkgpu_conn_desc;
int zkgpu_stark_conn_set(void *handle, uint32_t z, const zkgpu_conn_desc *d);
#define ZKGPU_CONN_MAX 16
typedef struct { uint32_t col, to_col; uint64_t row, to_row, value, to_value; } zkgpu_conn_break;
typedef struct { uint32_t col; uint64_t row, s_value; } zkgpu_conn_foreign;
typedef struct {
    uint32_t ran, z;  /* 1: the primitive ran; the product (index into zctx) */
    uint64_t n_broken, n_foreign, n_untargeted;
    zkgpu_conn_break breaks[ZKGPU_CONN_MAX];
    zkgpu_conn_foreign foreign[ZKGPU_CONN_MAX];
} zkgpu_conn_report;
int zkgpu_stark_conn_check(void *handle, uint32_t z, zkgpu_conn_report *out);
int zkgpu_stark_audit_conn(void *handle, uint32_t k, zkgpu_conn_report *out);

/* ---- the Fiat-Shamir transcript the prover runs on the host, as the
 * reference's class Transcript (transcript.hpp:14-37, transcript.cpp:4-88):
 * Poseidon-GL sponge, 8-element rate, 4-element capacity.  Host code only
 * (no GPU, no zkgpu_init needed).  Inputs are any u64 (reduced mod p, as
 * Goldilocks::Element); outputs are canonical. */
typedef struct zkgpu_transcript zkgpu_transcript;
zkgpu_transcript *zkgpu_transcript_create(void);                              /* Transcript() */
int zkgpu_transcript_put(zkgpu_transcript *t, const uint64_t *in, uint64_t n); /* put, :4-29 */
int zkgpu_transcript_get_fields1(zkgpu_transcript *t, uint64_t *out);         /* getFields1, :39-55 */
int zkgpu_transcript_get_field(zkgpu_transcript *t, uint64_t out[3]);         /* getField, :31-37 */
/* getPermutations, :57-88: n indices of nbits bits each (nbits <= 63) */
int zkgpu_transcript_get_permutations(zkgpu_transcript *t, uint64_t *res, uint64_t n, uint64_t nbits);
void zkgpu_transcript_destroy(zkgpu_transcript *t);

/* ---- one proof sharded over the GPUs of a node (BASELINE
 * configs[4]: "the same BatchProof trace column-sharded across 8 x MI355X").
 * The reference proves on one host (Starks::genProof, starks.cpp:9-404); this
 * is the multi-GPU form of the same proof, bit-identical to it.
 *
 * Point-to-point exchange between the ranks of a sharded prover: one grouped
 * batch of sends and receives of DEVICE buffers.  Operations with the same
 * peer and direction match in order on both sides; never peer == rank.  The
 * call returns once work enqueued afterwards on the zkgpu stream
 * (zkgpu_get_stream) sees the received bytes; the send buffers are not
 * modified before that either. */
typedef struct {
    int32_t peer;
    int32_t send; /* 1: send buf to peer; 0: receive into buf from peer */
    void *buf;    /* device pointer */
    uint64_t bytes;
} zkgpu_comm_op;

typedef struct {
    uint32_t rank, world; /* world a power of two */
    void *ctx;
    int (*exchange)(void *ctx, const zkgpu_comm_op *ops, uint32_t n_ops);
    /* optional (may be NULL): this rank has failed -- release the peers.  The
     * prover calls it when a sharded proof fails on this rank (a local error,
     * or an exchange it refuses), so that no peer waits for it: every later
     * exchange of the communicator then fails, on this rank at once and on the
     * peers at their next exchange (host shared memory) or within the
     * exchange deadline (RCCL). */
    int (*abort)(void *ctx);
} zkgpu_comm;

/* The RCCL implementation (ncclSend / ncclRecv inside ncclGroupStart/End,
 * enqueued on the zkgpu stream; xGMI between the GPUs of a node).  One rank
 * makes the id and hands it to the others (any side channel); every rank then
 * creates its communicator with its own rank.  librccl is opened at run time.
 * Each exchange waits for its transfers with a deadline (ZKGPU_COMM_TIMEOUT_S
 * seconds, default 120) while polling ncclCommGetAsyncError; on an error or
 * the deadline it calls ncclCommAbort (the transfer kernels exit) and fails,
 * and so does every later exchange: a rank whose peer failed or stopped
 * returns an error within the deadline instead of waiting forever. */
int zkgpu_comm_rccl_unique_id(uint8_t id[128]);
int zkgpu_comm_rccl_create(zkgpu_comm *comm, const uint8_t id[128], uint32_t world, uint32_t rank);
void zkgpu_comm_rccl_destroy(zkgpu_comm *comm);

/* Host shared-memory implementation for ranks that cannot use RCCL (several
 * processes sharing one GPU): POSIX shared memory `name` ("/..."), one
 * outbox of `capacity` bytes per rank and exchange, process-shared barriers.
 * Every rank calls create with the same name, world and capacity. */
int zkgpu_comm_host_create(zkgpu_comm *comm, const char *name, uint32_t world, uint32_t rank, uint64_t capacity);
void zkgpu_comm_host_destroy(zkgpu_comm *comm);

/* A prover whose extended (2n) domain is row-sharded over comm->world ranks:
 * rank r holds rows [r 2n/W, (r+1) 2n/W) of every extended section (plus the
 * next block's first 2^blowup rows), rows [r n/W, (r+1) n/W) of every n-domain
 * section (plus the next block's first rows up to the programs' largest row
 * shift), its share of the commitments' LDE columns, and the subtrees of its
 * rows.  Every rank calls the same functions in the same order
 * (witness / set_cm1 / set_const / set_publics / prove are collective) and
 * every rank's zkgpu_stark_prove returns the same proof, equal to
 * zkgpu_stark_create's.  comm is copied; comm->ctx must outlive the handle. */
int zkgpu_stark_create_sharded(void **handle, const zkgpu_stark_info *info, const zkgpu_comm *comm);
/* HBM one GPU holds at its peak for this description (its sections, the
 * transient setup copy of the constants, the library's workspaces): world 0
 * = zkgpu_stark_create, world W >= 1 = zkgpu_stark_create_sharded over W
 * ranks.  Host only, no GPU needed; both create calls fail loudly, before
 * allocating, when it exceeds the device's free memory. */
int zkgpu_stark_memory_plan(const zkgpu_stark_info *info, uint32_t world, uint64_t *bytes_per_gpu);
/* the same for a single-GPU prover (world 0) under memory plan RESIDENT or
 * LEAN (ZKGPU_MEM_*; AUTO = RESIDENT here: the choice needs a device) */
int zkgpu_stark_memory_plan_ex(const zkgpu_stark_info *info, uint32_t memory_plan, uint64_t *bytes);

#ifdef __cplusplus
}
#endif
#endif /* ZKGPU_STARK_H */
