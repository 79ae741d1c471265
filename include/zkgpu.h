/*
 * zkgpu.h -- C-ABI of libzkgpu, the MI355X (gfx950) STARK hot path for
 * zkevm-prover.  Plain pointers and sizes only; every function returns
 * ZKGPU_OK (0) or a negative error code, details in zkgpu_last_error().
 *
 * Two families:
 *   - host-pointer drop-ins with the reference's row-major buffers
 *     (stark_info.cpp:473-482 layout).  The library stages H2D, runs the HIP
 *     kernels on its device copy (column-major "SoA" internally), and copies
 *     the result back.  These are what the reference's C++ call sites bind to
 *     (see INTEGRATION.md for the adapter classes).
 *   - *_dev functions on device-resident column-major buffers (column c at
 *     ptr + c*ld), for traces kept in HBM across stages.  No host copies.
 *
 * Element type: Goldilocks u64, p = 2^64 - 2^32 + 1; inputs may be
 * non-canonical, outputs are canonical.  Extension elements are 3 u64.
 * The layout changes and copies (zkgpu_rows_to_cols_dev, zkgpu_cols_to_rows_dev,
 * zkgpu_copy_rows_dev, zkgpu_cols3_to_interleaved_dev) move words as they are.
 *
 * Leading dimensions: a column of a call over n rows needs ld >= n (the rows
 * in [n, ld) are neither read nor written).  The stage primitives below
 * return ZKGPU_ERR_ARG, with nothing queued, when an ld cannot hold the rows.
 *
 * Threading: one calling host thread per process/device (the reference calls
 * genProof from one thread, prover.cpp:182-255).  Kernels are enqueued on
 * the stream given to zkgpu_set_stream (default: the null stream); host-
 * pointer calls synchronise that stream before returning, *_dev calls do not.
 */
#ifndef ZKGPU_H
#define ZKGPU_H

#include <stdint.h>
#include "zkgpu_zxp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ZKGPU_OK 0
#define ZKGPU_ERR_HIP -1   /* HIP runtime error */
#define ZKGPU_ERR_ARG -2   /* invalid argument / unsupported size */
#define ZKGPU_ERR_INIT -3  /* zkgpu_init not called or failed */
#define ZKGPU_ERR_OOM -4   /* device allocation failed */

/* ---- lifecycle ------------------------------------------------------------
 * Replaces the implicit setup of the Goldilocks submodule objects:
 * NTT_Goldilocks(maxDomainSize, nThreads, extension) constructed at
 * starks.hpp:81-82 and friProve.cpp:100 (twiddle tables), plus the Poseidon
 * constant tables.  device = HIP device ordinal; device < 0 keeps the
 * initialised device, or uses the calling thread's current HIP device. */
int zkgpu_init(int device);
void zkgpu_release(void);
const char *zkgpu_last_error(void);
int zkgpu_set_stream(void *hip_stream);
/* the stream every zkgpu call is enqueued on (collectives of a sharded
 * prover are enqueued on it too, include/zkgpu_stark.h zkgpu_comm) */
void *zkgpu_get_stream(void);
int zkgpu_synchronize(void);
/* number of exported entry points (ABI self-check for tests) */
int zkgpu_abi_version(void);

/* ---- NTT ---------------------------------------------------------------
 * NTT_Goldilocks::NTT / INTT(Element *dst, Element *src, uint64_t size,
 * uint64_t ncols, Element *buffer, uint64_t nphase, uint64_t nblock)
 * -- starks.cpp:262 (INTT NE x 3), :285 (NTT NE x 6), :326-327 (INTT N x 3),
 * friProve.cpp:102.  Row-major n x ncols, natural order; INTT scales 1/n.
 * dst may equal src.  n must be a power of two <= 2^28. */
int zkgpu_gl_ntt(uint64_t *dst, const uint64_t *src, uint64_t n, uint64_t ncols, int inverse);

/* NTT_Goldilocks::extendPol(Element *output, Element *input, uint64_t N_Extended,
 * uint64_t N, uint64_t ncols, Element *buffer) -- starks.cpp:53,134,215.
 * out[i][c] = P_c(7 * omega_{n_ext}^i), P_c interpolating in[.][c] on <omega_n>.
 * Row-major in (n x ncols) and out (n_ext x ncols). */
int zkgpu_gl_extend_pol(uint64_t *out, const uint64_t *in, uint64_t n_ext, uint64_t n, uint64_t ncols);

/* device bytes extend_pol keeps in its grow-only workspaces for ncols
 * columns (column batches; for the host's memory plan, no GPU needed) */
uint64_t zkgpu_lde_workspace_bytes(uint64_t n, uint64_t n_ext, uint64_t ncols);
/* at most max_cols columns per extend_pol batch (0: the default, 2^31 words
 * of n_ext-row scratch): a smaller batch bounds the LDE workspace (and, in the
 * tests, exercises the column batching at small sizes).  Process-wide. */
void zkgpu_set_lde_batch_cols(uint64_t max_cols);

/* device-resident, column-major variants */
int zkgpu_gl_ntt_dev(uint64_t *dst, uint64_t ld_dst, const uint64_t *src, uint64_t ld_src, uint64_t n,
                     uint64_t ncols, int inverse);
int zkgpu_gl_extend_pol_dev(uint64_t *out, uint64_t ld_out, const uint64_t *in, uint64_t ld_in, uint64_t n_ext,
                            uint64_t n, uint64_t ncols);
/* extendPol in place (the same transform, starks.cpp:53,215): base holds
 * ncols n-row columns packed at ld n on entry and the ncols n_ext-row columns
 * at ld n_ext on return (base must hold ncols * n_ext words).  Column batches
 * run from the last down, each read whole into the LDE workspace before its
 * output is stored, so no column is overwritten before it is read; lets a
 * prover extend a section into the memory its n-domain values occupied
 * (host/starks.cpp, the lean memory plan).  Same values as extendPol
 * (starks.cpp:53,134,215) out of place. */
int zkgpu_gl_extend_pol_inplace_dev(uint64_t *base, uint64_t n_ext, uint64_t n, uint64_t ncols);
/* row-major <-> column-major on device (boundary layout change); ld >= nrows */
int zkgpu_rows_to_cols_dev(uint64_t *cols, uint64_t ld, const uint64_t *rows, uint64_t nrows, uint64_t ncols);
int zkgpu_cols_to_rows_dev(uint64_t *rows, const uint64_t *cols, uint64_t ld, uint64_t nrows, uint64_t ncols);

/* ---- Poseidon-GL --------------------------------------------------------
 * PoseidonGoldilocks::hash_full_result(Element out[12], const Element in[12])
 * -- transcript.cpp:23,46.  Computed on the GPU. */
int zkgpu_gl_poseidon_full(uint64_t out[12], const uint64_t in[12]);
/* The same permutation on the host CPU (no GPU, no zkgpu_init): the
 * transcript's (Transcript::put/getFields, transcript.cpp:18-24 ->
 * PoseidonGoldilocks::hash_full_result), where one serial permutation sits on
 * the critical path and a GPU launch would only add latency. */
int zkgpu_gl_poseidon_full_host(uint64_t out[12], const uint64_t in[12]);
/* PoseidonGoldilocks::hash(Element out[4], const Element in[12]) */
int zkgpu_gl_poseidon_hash(uint64_t out[4], const uint64_t in[12]);
/* PoseidonGoldilocks::linear_hash(Element *out, Element *in, uint64_t size)
 * -- main_sm/fork_9/main_exec (utils.cpp:708).  One input row. */
int zkgpu_gl_linear_hash(uint64_t out[4], const uint64_t *in, uint64_t size);
/* batched permutation on device: in/out are n x 12 (full) or out n x 4 */
int zkgpu_gl_poseidon_batch_dev(uint64_t *out, const uint64_t *in, uint64_t n, int full);

/* ---- Merkle tree GL ----------------------------------------------------
 * MerklehashGoldilocks::getTreeNumElements(nrows) (stark_info.hpp:332,
 * build_const_tree.cpp:566-569): 4*nrows + 4*(nrows-1). */
uint64_t zkgpu_gl_merkle_num_elements(uint64_t nrows);
/* PoseidonGoldilocks::merkletree{,_avx,_avx512}(Element *tree, Element *input,
 * uint64_t ncols, uint64_t nrows) -- merkleTreeGL.cpp:37-44,
 * build_const_tree.cpp:582.  Row-major source; nrows a power of two. */
int zkgpu_gl_merkletree(uint64_t *nodes, const uint64_t *src, uint64_t ncols, uint64_t nrows);
/* device-resident: src column-major (ld), nodes on device */
int zkgpu_gl_merkletree_dev(uint64_t *nodes, const uint64_t *src, uint64_t ld, uint64_t ncols, uint64_t nrows);
/* the same tree over a section held in two regions: columns [0, split) at
 * src + c*ld, columns [split, ncols) at src2 + (c - split)*ld (split a
 * multiple of 8: the linear hash absorbs 8 columns at a time).  The lean
 * memory plan's stage-1 commit (host/starks.cpp); same nodes as the
 * reference's merkelize of the whole section (merkleTreeGL.cpp:37-44). */
int zkgpu_gl_merkletree2_dev(uint64_t *nodes, const uint64_t *src, const uint64_t *src2, uint64_t ld, uint64_t split,
                             uint64_t ncols, uint64_t nrows);
/* The same tree built while its section arrives in column chunks: the linear
 * hash's 4-word capacity is carried between calls in the tree's leaf slots
 * (the first 4*nrows words of nodes), so after the last chunk they hold the
 * leaf digests and zkgpu_gl_merkle_finish_dev adds the levels above them.
 * absorb columns [col0, col0+ncols) of a total_cols-wide section into the
 * leaf sponge held in nodes[0, 4*nrows); src points at column col0.
 * col0 % 8 == 0; ncols % 8 == 0 unless this is the last chunk.  A section of
 * total_cols <= 4 (copied, not hashed) comes as one chunk. */
int zkgpu_gl_merkle_leaves_absorb_dev(uint64_t *nodes, const uint64_t *src, uint64_t ld, uint64_t col0, uint64_t ncols,
                                      uint64_t total_cols, uint64_t nrows);
/* the tree levels over finished leaves (merkle_levels) */
int zkgpu_gl_merkle_finish_dev(uint64_t *nodes, uint64_t nrows);
/* device-resident, row-major source (FRI trees: friProve.cpp:117-121) */
int zkgpu_gl_merkletree_rows_dev(uint64_t *nodes, const uint64_t *src, uint64_t ncols, uint64_t nrows);
/* ---- constant tree (tools/starkpil/bctree) -----------------------------
 * Element count of a const-tree file: header 2 + nPols*nExt + tree
 * (build_const_tree.cpp:566-569). */
uint64_t zkgpu_const_tree_num_elements(uint64_t n_pols, uint32_t n_bits_ext);
/* build_const_tree.cpp:553-603 (GL hash): interpolate (extendPol of the
 * row-major N x nPols constant pols to nExt rows) + PoseidonGoldilocks::
 * merkletree, written in the file layout [nPols, nExt, LDE row-major,
 * tree nodes]; the verkey constRoot is the last 4 elements.  Host pointers. */
int zkgpu_build_const_tree(uint64_t *tree_out, const uint64_t *const_pols, uint64_t n_pols, uint32_t n_bits,
                           uint32_t n_bits_ext);

/* ---- executor hand-off ------------------------------------------------
 * Load a host row-major section (the committed-pols buffer the executor
 * fills, CommitPols stride = width, commit_pols.hpp:18,1735-1737; read by
 * prover.cpp:94-116) into device column-major storage (column c at
 * cols + c*ld), streamed in row blocks: each block's H2D copy runs on a copy
 * stream while the previous block is transposed, so a pinned (registered)
 * source moves at link speed.  register_host = 1 page-locks `rows` for the
 * duration of the call (hipHostRegister). */
int zkgpu_load_rows_dev(uint64_t *cols, uint64_t ld, const uint64_t *rows, uint64_t nrows, uint64_t ncols,
                        uint64_t block_rows, int register_host);
/* The same load of the column window [col0, col0+wcols) of the ncols-wide
 * rows, into columns cols + c*ld (c < wcols; the columns outside the window
 * are not touched): each block's copy is a strided one (host pitch ncols
 * words).  The whole width is zkgpu_load_rows_dev. */
int zkgpu_load_rows_window_dev(uint64_t *cols, uint64_t ld, const uint64_t *rows, uint64_t nrows, uint64_t ncols,
                               uint64_t col0, uint64_t wcols, uint64_t block_rows, int register_host);
/* Windows of one host buffer (nrows x ncols), queued one after another from
 * the caller's thread on streams of the loader's own (stage: caller-owned
 * device buffer, two halves of at least one window row each; register_host
 * page-locks `rows` from open to close).  zkgpu_load_stream_window returns
 * with the window's copies and transposes queued and with the library stream
 * made to wait for them: work queued on it afterwards sees the columns, while
 * later windows cross PCIe beside it (a pinned or registered source; the
 * copies of a pageable one block the caller, which stays correct).  The
 * first window is ordered after everything queued on the library stream at
 * open.  zkgpu_load_stream_close waits for what was queued and frees the
 * loader, also after a failed window.  The prover's streamed stage 1
 * (zkgpu_stark_prove_from_rows) runs on it.  ZKGPU_STREAM_FAIL_BATCH=k
 * (tests): window k (from 0) fails before anything of it is queued. */
int zkgpu_load_stream_open(void **loader, const uint64_t *rows, uint64_t nrows, uint64_t ncols, uint64_t *stage,
                           uint64_t stage_bytes, int register_host);
int zkgpu_load_stream_window(void *loader, uint64_t *cols, uint64_t ld, uint64_t col0, uint64_t wcols);
int zkgpu_load_stream_close(void *loader);
/* The same load in the background: a host thread of the library runs the
 * block loop on streams of its own (stage: caller-owned device buffer of at
 * least zkgpu_load_rows_stage_bytes bytes), so kernels on the library stream
 * -- the previous proof -- run while the trace crosses PCIe.  `rows`, `cols`
 * and `stage` stay untouched by the caller until zkgpu_load_wait(ticket)
 * returns (the load's status, and on failure the loader's message in
 * zkgpu_last_error() of the waiting thread; the ticket is freed).  The load
 * is ordered after everything already queued on the library stream (e.g. the
 * zeroing of freshly allocated `cols` / `stage`).  No reference
 * counterpart: the reference's batch prover loads each trace before its
 * genProof (prover.cpp:94-116). */
uint64_t zkgpu_load_rows_stage_bytes(uint64_t nrows, uint64_t ncols, uint64_t block_rows);
int zkgpu_load_rows_async(uint64_t *cols, uint64_t ld, const uint64_t *rows, uint64_t nrows, uint64_t ncols,
                          uint64_t block_rows, uint64_t *stage, uint64_t stage_bytes, void **ticket);
int zkgpu_load_wait(void *ticket);

/* MerkleTreeGL::getGroupProof(Element *proof, uint64_t idx) for nq queries at
 * once -- merkleTreeGL.cpp:12-35, friProve.cpp:195-232.
 * vals_out: nq x ncols, sibs_out: nq x log2(nrows) x 4 (host pointers);
 * src column-major on device (ld), nodes on device.  ZKGPU_ERR_ARG, with
 * nothing queued, when nrows is not a power of two or an index is >= nrows. */
int zkgpu_gl_merkle_open_dev(uint64_t *vals_out, uint64_t *sibs_out, const uint64_t *nodes, const uint64_t *src,
                             uint64_t ld, uint64_t ncols, uint64_t nrows, const uint64_t *idx, uint64_t nq);

/* ---- FRI -----------------------------------------------------------------
 * One fold step of FRIProve::prove (friProve.cpp:20-108), device-resident:
 * pol has 2^pol_bits ext elements (interleaved, 3 u64 each), out 2^out_bits.
 * special_x: host pointer to 3 u64; shift_inv: polShiftInv of this step. */
int zkgpu_fri_fold_dev(uint64_t *out, const uint64_t *pol, uint32_t pol_bits, uint32_t out_bits,
                       const uint64_t special_x[3], uint64_t shift_inv);
/* The same fold for output groups [g0, g0 + ngroups) only, reading those
 * groups' getTransposed rows (row g - g0 = the 2^(pol_bits - out_bits)
 * elements pol[g + i 2^out_bits], 3 u64 each: the layout
 * zkgpu_fri_transpose_dev writes with transpose_bits = out_bits); out gets
 * the ngroups folded elements.  The row-sharded prover's first fold, each
 * rank on its block of groups (friProve.cpp:44-108 restricted to g). */
int zkgpu_fri_fold_rows_dev(uint64_t *out, const uint64_t *rows, uint64_t g0, uint64_t ngroups, uint32_t pol_bits,
                            uint32_t out_bits, const uint64_t special_x[3], uint64_t shift_inv);
/* FRIProve::getTransposed (friProve.cpp:252-270), ext elements, device */
int zkgpu_fri_transpose_dev(uint64_t *aux, const uint64_t *pol, uint64_t degree, uint32_t transpose_bits);

/* ---- calculateH1H2 over row-sharded f / t --------------------------------
 * Polinomial::calculateH1H2_opt1/opt3 (polinomial.hpp:349-583, starks.cpp:
 * 104-127) when W ranks each hold rows [row0, row0 + nrows) of f and t (the
 * row-sharded prover, host/sharded_starks.hpp; the same h1 / h2 as
 * zkgpu_h1h2_dev on the whole columns).  Records are 5 u64 {k0, k1, k2,
 * global row, val}: a rank's distinct t keys (largest row, val = ~0) and f
 * keys (smallest row, val = count), each sent to the rank owning its key.
 *   route:  dedupe the rank's rows, write the records bucketed by owner into
 *           recs (owner order, t records first in each bucket; at most cap
 *           records), n_t / n_f (host, world entries) = the bucket sizes
 *   owner:  over every record this rank owns (all ranks' buckets for it,
 *           concatenated, each t-first): ret[k] = the f count summed over the
 *           ranks for t record k if its row is the key's largest, else 0;
 *           missing_row = the smallest f row whose key has no t row (~0 if
 *           none: the reference's "Number not included")
 *   counts: the sender, ret aligned with its own recs (nsent records):
 *           cnt[j] = 1 + ret of row j's record, start = exclusive scan of cnt
 *           (the rank's multiset positions, relative); total (host) = sum
 *   deal:   seg[c * seg_ld + start[j] + m] = t[c * t_ld + j], m < cnt[j]
 *   place:  buf holds multiset positions [pos0, pos0 + len) (column c at
 *           buf + c * buf_ld): even positions p to h1, odd to h2, at local
 *           row p / 2 - row0. */
int zkgpu_h1h2_shard_route(uint64_t *recs, uint64_t cap, uint32_t *n_t, uint32_t *n_f, const uint64_t *f,
                           uint64_t f_ld, const uint64_t *t, uint64_t t_ld, uint64_t nrows, uint64_t row0, uint32_t dim,
                           uint32_t world);
int zkgpu_h1h2_shard_owner(uint64_t *ret, const uint64_t *recs, uint64_t nrec, uint32_t dim, uint64_t *missing_row);
int zkgpu_h1h2_shard_counts(uint32_t *start, uint32_t *cnt, uint64_t *total, const uint64_t *sent, const uint64_t *ret,
                            uint64_t nsent, uint64_t nrows, uint64_t row0);
int zkgpu_h1h2_shard_deal(uint64_t *seg, uint64_t seg_ld, const uint64_t *t, uint64_t t_ld, const uint32_t *start,
                          const uint32_t *cnt, uint64_t nrows, uint32_t dim);
int zkgpu_h1h2_shard_place(uint64_t *h1, uint64_t h1_ld, uint64_t *h2, uint64_t h2_ld, const uint64_t *buf,
                           uint64_t buf_ld, uint64_t pos0, uint64_t len, uint64_t row0, uint32_t dim);

/* ---- device memory (the host orchestrator owns HBM through these) -------- */
int zkgpu_dev_malloc(void **ptr, uint64_t bytes);
/* free / total HBM of the bound device (hipMemGetInfo) */
int zkgpu_device_memory(uint64_t *free_bytes, uint64_t *total_bytes);
int zkgpu_dev_free(void *ptr);
int zkgpu_memcpy_h2d(void *dst, const void *src, uint64_t bytes);
int zkgpu_memcpy_d2h(void *dst, const void *src, uint64_t bytes);
int zkgpu_memcpy_d2d(void *dst, const void *src, uint64_t bytes);
int zkgpu_memset_dev(void *dst, int value, uint64_t bytes);

/* ---- STARK stage primitives (device-resident, column-major sections) ------
 * Section table for the expression programs: base pointer + leading
 * dimension per eSection (include/zkgpu_zxp.h SEC_*), the device analogue of
 * the reference's mapOffsets/mapSectionsN (stark_info.cpp:473-482). */
typedef struct {
    uint64_t *sec[12];
    uint64_t ld[12];    /* leading dimension = rows allocated per column */
    uint32_t ncols[12]; /* columns allocated (bounds-checked at launch) */
} zkgpu_sections;

/* Executor stand-in for synthetic traces: column cols[k] of a column-major
 * buffer gets the deterministic pseudo-random elements rand(seed, stream, col, row).
 * ZKGPU_ERR_ARG when ncols > 65535 or nrows > ld. */
int zkgpu_rand_cols_dev(uint64_t *base, uint64_t ld, const uint32_t *cols, uint32_t ncols, uint64_t nrows,
                        uint64_t seed, uint64_t stream);
/* the same for a row block of a 2^log_n-row domain: local row r of the
 * buffer gets global row (row0 + r) mod 2^log_n (halo rows after a block wrap
 * to the domain's first rows) */
int zkgpu_rand_cols_rows_dev(uint64_t *base, uint64_t ld, const uint32_t *cols, uint32_t ncols, uint64_t row0,
                             uint64_t nrows, uint32_t log_n, uint64_t seed, uint64_t stream);

/* Rows of selected columns between column-major device buffers -- the halo
 * refresh, shifted-store spill and block copies of the row-sharded prover
 * (host/sharded_starks.hpp): for k < ncols, j < nrows
 *   dst[dcol_k * dst_ld + dst_row0 + j] = src[scol_k * src_ld + (src_row0 + j) mod 2^src_log_mod]
 * with dcol_k = dst_cols[k] (k when dst_cols is NULL), likewise scol_k;
 * src_log_mod = 0: no wrap.  The column lists are host arrays. */
int zkgpu_copy_rows_dev(uint64_t *dst, uint64_t dst_ld, uint64_t dst_row0, const uint32_t *dst_cols,
                        const uint64_t *src, uint64_t src_ld, uint64_t src_row0, uint32_t src_log_mod,
                        const uint32_t *src_cols, uint32_t ncols, uint64_t nrows);

/* out[j * ncols + c] = src[c * ld + rows[j]] for j < nrows, c < ncols:
 * rows `rows` (device array, any order, repeats allowed, each < ld) of a
 * column-major section into a row-major block (the layout
 * oc_parser_eval_rows / the reference's pols take).  Enqueued on the zkgpu
 * stream.  A row index >= ld is not read: its block row is zero. */
int zkgpu_gather_rows_dev(uint64_t *out, const uint64_t *src, uint64_t ld, uint32_t ncols, const uint64_t *rows,
                          uint64_t nrows);

/* The rows of a column-major section that are not zero (the prover's constraint check,
 * include/zkgpu_stark.h zkgpu_stark_check_*).
 * out (device, 1 + max_rows words): out[0] = number of rows i < n with cols[c*ld + i] != 0 (mod p) for
 * some c < ncols; out[1 + k] = the k-th lowest such row, ascending, UINT64_MAX past the last.
 * Inputs may be non-canonical (p and 0 are both zero).  Enqueued on the library stream, no host
 * synchronisation.  ZKGPU_ERR_ARG: ld < n, max_rows > 4096, null pointers; n = 0 or ncols = 0 write count 0.
 * The result does not depend on the launch geometry: per 1024-row block counts, then one workgroup
 * that scans them and re-reads only the blocks holding the lowest max_rows hits. */
int zkgpu_nonzero_rows_dev(uint64_t *out, const uint64_t *cols, uint64_t ld, uint32_t ncols,
                           uint64_t n, uint32_t max_rows);

/* Steps::step*_parser_first (steps.hpp:21-58; used at starks.cpp:73,155,193,
 * 241,371): evaluate one expression program (include/zkgpu_zxp.h) over every
 * row of its domain (2^log_dom rows).  instr/opnd are host arrays (uploaded),
 * challenges (8 x 3), publics and evals are host arrays; xdiv/xdivw are
 * device arrays (2n x 3 interleaved) for the FRI program, else NULL;
 * extend_bits sizes zhInv (zhInv.cpp:7-31); x_start = 1 (n domain) or 7 (2n). */
int zkgpu_zxp_eval_dev(const void *instr, uint32_t n_instr, const void *opnd, uint32_t n_opnd, uint32_t n_tmp1,
                       uint32_t n_tmp3, const zkgpu_sections *sections, uint32_t log_dom, const uint64_t *challenges,
                       const uint64_t *publics, uint32_t n_publics, const uint64_t *evals, uint32_t n_evals,
                       const uint64_t *xdiv, const uint64_t *xdivw, uint32_t extend_bits, uint64_t x_start);

/* The same over ONE ROW BLOCK of a row-sharded domain (the
 * quotient and FRI programs run on the rows a GPU owns after the column ->
 * row exchange).  Rows 0 .. 2^log_rows - 1 of every section are evaluated;
 * x_i = x_start * w_{2^log_domain}^i (x_start = 7 * w^row0 for a block
 * starting at global row row0), zhInv uses N = 2^(log_domain - extend_bits),
 * and a read at row shift s >= 0 does not wrap: the caller stores the next
 * block's first s rows (the halo) after the block, so every section's
 * ld >= 2^log_rows + s.  A store at row shift s likewise writes local row
 * i + s: its last s rows land in the halo, and the caller moves them to the
 * next block (host/sharded_starks.hpp).
 * The call takes x_start, not row0, so two things are the caller's duty and
 * cannot be checked here.  The block must start at a multiple of
 * 2^extend_bits: zhInv has 2^extend_bits entries and is indexed by the LOCAL
 * row (i mod 2^extend_bits), which is the global row's entry only then.  And
 * xdiv / xdivw are read at local row i (words 3 i .. 3 i + 2): the caller
 * passes them advanced to the block's first row (base + 3 row0).
 * ZKGPU_ERR_ARG, nothing queued: log_rows > log_domain, a read or store at a
 * negative row shift, a section whose ld is below 2^log_rows + s for a column
 * read or stored at shift s. */
int zkgpu_zxp_eval_block_dev(const void *instr, uint32_t n_instr, const void *opnd, uint32_t n_opnd, uint32_t n_tmp1,
                             uint32_t n_tmp3, const zkgpu_sections *sections, uint32_t log_rows, uint32_t log_domain,
                             const uint64_t *challenges, const uint64_t *publics, uint32_t n_publics,
                             const uint64_t *evals, uint32_t n_evals, const uint64_t *xdiv, const uint64_t *xdivw,
                             uint32_t extend_bits, uint64_t x_start);

/* Host-only compiler behind zkgpu_zxp_eval_dev (include/zkgpu_zxp.h,
 * "compiled programs"): folds the row-constant operands (challenges 8 x 3,
 * publics, evals n_evals x 3, literals) into linear-combination instructions
 * with at most max_terms terms each (0 = default 64, cap 256) and packs the
 * temporaries.  The output arrays stay valid until the next call on the same
 * thread.  No GPU needed; used by the tests to check the compiled program
 * against the source program on the CPU oracle. */
int zkgpu_zxp_compile(const void *instr, uint32_t n_instr, const void *opnd, uint32_t n_opnd, uint32_t n_tmp1,
                      uint32_t n_tmp3, const uint64_t *challenges, const uint64_t *publics, uint32_t n_publics,
                      const uint64_t *evals, uint32_t n_evals, uint32_t max_terms, zxp_compiled *out);

/* A quotient program (step42ns) re-targeted to the trace domain (csrc/zxp_n_domain.cpp): the
 * combination C it forms before its final "x ZI" is zero on every row of <omega_n> exactly when the
 * trace satisfies every identity (with overwhelming probability over the combination challenge).
 * Reads of SEC_CM1/CM2/CM3/CONST_2NS become reads of the matching _N section, their row shift (a
 * multiple of 2^extend_bits, either sign) divided by 2^extend_bits (next = 2^extendBits -> 1,
 * steps.hpp); SEC_Q_2NS stays, destination only, shift 0 (the caller points that section-table
 * entry at n-row storage); ZXP_ZI becomes ZXP_LIT 1 and is accepted only as a factor of a ZXP_MUL
 * stored to a SEC_Q_2NS column, of which there must be one; X, TMP1/3, LIT, CHAL, PUB are unchanged;
 * everything else (EVAL, XDIV, XDIVW, any other section, a read of SEC_Q_2NS, unknown kinds,
 * indices out of range) is ZKGPU_ERR_ARG with a message naming the operand or instruction.  Then
 * evaluate with zkgpu_zxp_eval_dev at log_dom = n_bits, x_start = 1, extend_bits = 0.
 * opnd_out: n_opnd operands; the instruction list is unchanged.  No GPU needed. */
int zkgpu_zxp_to_n_domain(zxp_operand *opnd_out, const zxp_instr *instr, uint32_t n_instr,
                          const zxp_operand *opnd, uint32_t n_opnd, uint32_t extend_bits);

/* The constraint combination of a quotient program taken apart into its terms (csrc/zxp_split.cpp,
 * which states the rule).  instr/opnd: step42ns as given or as rewritten by zkgpu_zxp_to_n_domain;
 * chal: the index of the combination challenge (4).  Outputs: a TAPPED program -- the source's
 * instructions that touch no combination, verbatim and in order, and where term k joins the
 * combination "COPY COL3(SEC_Q_2NS, 3k) <- x"; the final store to q is dropped -- over an operand
 * table that is the source's followed by the taps' operands, and the term table.  Per row the tapped
 * program's 3 * n_terms output columns hold the values v_k with
 *     C = sum over the terms k that are not dead of (-1)^negated_k * alpha^exponent_k * v_k
 * exactly, C being the value the source stores to q (without its factor ZI).  The k-th term is the
 * k-th identity folded, in the producer's order; terms[k].instr is the source instruction where it
 * joined.  Buffer sizes (at most two taps per source instruction): instr_out 2 * n_instr, opnd_out
 * n_opnd + 2 * n_instr + 1, terms 2 * n_instr; the counts written are what was used.  The temp
 * counts are the source's.  ZKGPU_ERR_ARG with a message naming the instruction: a combination
 * multiplied by anything but the challenge (ZI or the literal 1 at the store to q excepted; a product
 * into a TMP3 slot whose value reaches no combination and no column is dropped instead), written to
 * a TMP1 slot, to a column other than COL3(SEC_Q_2NS, 0, shift 0) or there by an ADD / SUB / product
 * by the challenge, two combinations that share a term added, a store to SEC_Q_2NS that is free of
 * the challenge, a second store to q or none, indices out of range.  No GPU needed. */
int zkgpu_zxp_split_constraints(zxp_instr *instr_out, uint32_t *n_instr_out, zxp_operand *opnd_out,
                                uint32_t *n_opnd_out, zxp_split_term *terms, uint32_t *n_terms,
                                const zxp_instr *instr, uint32_t n_instr, const zxp_operand *opnd,
                                uint32_t n_opnd, uint32_t chal);

/* zkgpu_zxp_eval_dev at a LIST OF ROWS held in device memory: for every j < n_rows with
 * rows[j] < 2^log_dom the program is evaluated at row i = rows[j] -- column reads at
 * (i + shift) mod 2^log_dom of the section, X / ZI / XDIV / XDIVW at i -- and its column STORES go to
 * index j of the destination column, so a section the program stores to is compact: ld >= n_rows.
 * An entry rows[j] >= 2^log_dom writes nothing at index j (zkgpu_nonzero_rows_dev pads its list
 * with UINT64_MAX); the list may be unsorted and hold repeats.  The other arguments are those of
 * zkgpu_zxp_eval_dev.  Always the interpreter (k_zxp_eval_rows, csrc/stark.hip), after the same
 * argument checks, compile and LDS bound; enqueued on the library stream with NO host
 * synchronisation (the records go up from pinned staging buffers that are reused once their copy
 * has completed).  ZKGPU_ERR_ARG, nothing queued: a section that is both read and stored to, a
 * store at a row shift, a store section with ld < n_rows, n_rows > 4096, null rows.  n_rows = 0
 * queues nothing. */
int zkgpu_zxp_eval_rows_dev(const void *instr, uint32_t n_instr, const void *opnd, uint32_t n_opnd, uint32_t n_tmp1,
                            uint32_t n_tmp3, const zkgpu_sections *sections, uint32_t log_dom,
                            const uint64_t *challenges, const uint64_t *publics, uint32_t n_publics,
                            const uint64_t *evals, uint32_t n_evals, const uint64_t *xdiv, const uint64_t *xdivw,
                            uint32_t extend_bits, uint64_t x_start, const uint64_t *rows, uint32_t n_rows);

/* Diagnostics for the run-time compiled expression kernels (csrc/zxp_jit.hip):
 * compile a program exactly as zkgpu_zxp_eval_dev does and write the
 * generated straight-line HIP kernel source into buf (truncated to buflen);
 * with rtc_check != 0 also compile it for gfx950 with hiprtc (or find it in
 * the on-disk code-object cache; rtc_check = 2 also writes the code object to
 * $ZKGPU_ZXP_JIT_DUMP).  rtc_check = 3 only queries the cache: returns 1 when
 * the compiled kernel is on disk, 0 when not.  No GPU needed.
 * Returns the source length (>= 0) or an error code. */
int zkgpu_zxp_jit_source(const void *instr, uint32_t n_instr, const void *opnd, uint32_t n_opnd, uint32_t n_tmp1,
                         uint32_t n_tmp3, const uint64_t *challenges, const uint64_t *publics, uint32_t n_publics,
                         const uint64_t *evals, uint32_t n_evals, char *buf, uint64_t buflen, int rtc_check);

/* Polinomial::calculateZ(z, num, den) (polinomial.hpp:586-607), F_p^3 columns
 * (3 consecutive columns of ld each).  *closes = 1 iff z[n-1]*num[n-1]/den[n-1] == 1
 * (the reference's zkassert).  ZKGPU_ERR_ARG when z_ld, num_ld or den_ld < n
 * (the block and batched forms alike).  A zero denominator is outside the
 * contract (the reference inverts the whole column at once, this per thread:
 * they differ there). */
int zkgpu_calculate_z_dev(uint64_t *z, uint64_t z_ld, const uint64_t *num, uint64_t num_ld, const uint64_t *den,
                          uint64_t den_ld, uint64_t n, int *closes);
/* One row block of the same grand product (the row-sharded prover: each rank
 * its block, then a scan of the W block totals): z[i] = z0 * prod_{j<i}
 * num[j] / den[j] for i < n; total (host, canonical) = z0 * prod_{j<n}
 * num[j] / den[j].  calculateZ over the whole domain is z0 = 1, closes iff
 * total == 1. */
int zkgpu_calculate_z_block_dev(uint64_t *z, uint64_t z_ld, const uint64_t *num, uint64_t num_ld, const uint64_t *den,
                                uint64_t den_ld, uint64_t n, const uint64_t z0[3], uint64_t total[3]);
/* Every grand product of a stage (starks.cpp:165-189: calculateZ per
 * permutation / plookup / connection context) in one round trip: request k is
 * zkgpu_calculate_z_dev's (z, z_ld, num, num_ld, den, den_ld) over the same n;
 * closes[k] as there.  One read-back of the nz totals instead of nz. */
typedef struct zkgpu_z_req {
    uint64_t *z;
    uint64_t z_ld;
    const uint64_t *num;
    uint64_t num_ld;
    const uint64_t *den;
    uint64_t den_ld;
} zkgpu_z_req;
int zkgpu_calculate_z_many_dev(const zkgpu_z_req *req, uint32_t nz, uint64_t n, int *closes);

/* Starks::evmap (starks.cpp:556-669): evals[e] = sum_{k<n} L(k) * pol_e[k << extend_bits],
 * L = lev or lpev (device, 3 columns of ld l_ld).  cols = host array of device
 * column pointers (first column of each polynomial), lds / dims / primes per
 * entry.  evals_out: host (n_ev x 3).  A row block of longer columns is the
 * same call with the pointers advanced (lev + k0, col + (k0 << extend_bits))
 * and the leading dimensions kept.  ZKGPU_ERR_ARG, with nothing queued, when
 * l_ld < n or when the lds[e] of a dim-3 entry cannot hold the
 * ((n - 1) << extend_bits) + 1 rows read (a dim-1 entry's is not used);
 * n = 0 writes zero evaluations and launches nothing. */
int zkgpu_evmap_dev(uint64_t *evals_out, const uint64_t *const *cols, const uint64_t *lds, const uint32_t *dims,
                    const uint32_t *primes, uint32_t n_ev, const uint64_t *lev, const uint64_t *lpev, uint64_t l_ld,
                    uint64_t n, uint32_t extend_bits);

/* xDivXSubXi / xDivXSubWXi (starks.cpp:344-366) over x_k = 7 w_{2n}^k, k < 2^n_bits_ext;
 * w = Goldilocks::w(n_bits).  Outputs interleaved (2n x 3), device. */
int zkgpu_xdivxsub_dev(uint64_t *xdiv, uint64_t *xdivw, const uint64_t xi[3], uint32_t n_bits, uint32_t n_bits_ext);
/* The same for rows [row0, row0 + nrows) of the extended domain only, written
 * at their places (xdiv + 3 row0 ...): a row-sharded prover's block. */
int zkgpu_xdivxsub_rows_dev(uint64_t *xdiv, uint64_t *xdivw, const uint64_t xi[3], uint32_t n_bits,
                            uint32_t n_bits_ext, uint64_t row0, uint64_t nrows);
/* LEv / LpEv (starks.cpp:308-324: INTT_N of the powers of xi and of w_N xi),
 * rows [row0, row0 + nrows) in closed form: LEv[k] = ((1 - xi^N) / N) x_k /
 * (x_k - xi) with x_k = w_N^k (LpEv: w_N xi) -- the same field values, row by
 * row, so each rank computes only its own rows.  lev / lpev: 3 columns of
 * leading dimension ld holding rows row0.. at offset 0.  Fails
 * (ZKGPU_ERR_ARG) when xi lies in the base field, where a denominator may
 * vanish: interpolate (zkgpu_ext_powers_dev + zkgpu_gl_ntt_dev) instead. */
int zkgpu_lagrange_xi_rows_dev(uint64_t *lev, uint64_t *lpev, uint64_t ld, const uint64_t xi[3], uint32_t n_bits,
                               uint64_t row0, uint64_t nrows);

/* base^k for k < n into 3 columns of ld >= n (LEv / LpEv, starks.cpp:308-324) */
int zkgpu_ext_powers_dev(uint64_t *out, uint64_t ld, const uint64_t base[3], uint64_t n);

/* cols[c][k] *= base^k for k < n, c < ncols (canonical outputs): the coset
 * shift of coefficient vectors (the shift^i multiply of
 * NTT_Goldilocks::extendPol, starks.cpp:53), used to move the quotient
 * pieces between coset-scaled and plain coefficients. */
int zkgpu_scale_by_powers_dev(uint64_t *cols, uint64_t ld, uint32_t ncols, uint64_t n, uint64_t base);

/* quotient split (starks.cpp:266-281): qq2 col 3p+d row k = qq1 col d row pN+k * shift_in^p, k < n;
 * ld2 >= n and ld1 >= q_deg * n (ZKGPU_ERR_ARG otherwise) */
int zkgpu_qsplit_dev(uint64_t *qq2, uint64_t ld2, const uint64_t *qq1, uint64_t ld1, uint64_t n, uint32_t q_deg,
                     uint64_t shift_in);
/* the same for dim input columns into output columns stride*p + d (d < dim
 * <= stride): a column owner of the row-sharded prover splits its one
 * quotient column (dim 1, stride 3) */
int zkgpu_qsplit_cols_dev(uint64_t *qq2, uint64_t ld2, const uint64_t *qq1, uint64_t ld1, uint64_t n, uint32_t q_deg,
                          uint64_t shift_in, uint32_t dim, uint32_t stride);

/* plookup h1/h2 (Polinomial::calculateH1H2_opt1 / _opt3, polinomial.hpp:349-583,
 * called at starks.cpp:104-127): f, t, h1, h2 are n-row columns of dimension
 * dim (1, or 3 = three column-major components ld apart).  Every table row
 * starts with multiplicity 1; each f value adds one to the LAST table row with
 * the same (canonical) value; the multiset in table order is dealt
 * alternately into h1 and h2.  An f value absent from t returns ZKGPU_ERR_ARG
 * ("Number not included", the reference exits) with *missing_row = the first
 * such f row; otherwise *missing_row = UINT64_MAX. */
int zkgpu_h1h2_dev(uint64_t *h1, uint64_t h1_ld, uint64_t *h2, uint64_t h2_ld, const uint64_t *f, uint64_t f_ld,
                   const uint64_t *t, uint64_t t_ld, uint64_t n, uint32_t dim, uint64_t *missing_row);

/* Multiset comparison of two n-row columns a and b of dimension dim (1, or 3 = three column-major
 * components one leading dimension apart, as zkgpu_h1h2_dev): the distinct values whose
 * multiplicity in a differs from their multiplicity in b.  A value is the canonical dim-tuple
 * (v and v + p are the same value).  What a grand product that does not close is asked
 * (host/starks.cpp z_all): for a permutation check num = f + gamma, den = t + gamma the answer is
 * the offending values themselves.
 * out (device, 2 * (1 + 3 * max_vals) words), two blocks of 1 + 3 * max_vals words:
 *   block A  out[0] = the number of distinct values that occur in a with unequal counts, then
 *            max_vals triples {the value's first row in a, its count in a, its count in b}
 *            ordered by that row, ascending; UINT64_MAX, 0, 0 past the last
 *   block B  the same for the values that occur in b: {first row in b, count in a, count in b}
 * (a value on both sides with unequal counts is in both blocks).  Reported by value, not by row:
 * a default value on millions of rows with one copy too many is ONE entry.
 * The result does not depend on the launch geometry or on which thread claims a table slot:
 * counts are atomic sums, first rows atomic minima, and the lists come from the reduction of
 * zkgpu_nonzero_rows_dev over a flag on each value's first row.  Enqueued on the library stream,
 * no host synchronisation; rows [n, ld) are not read; a == b is allowed.  ZKGPU_ERR_ARG, nothing
 * queued: a_ld < n or b_ld < n, dim not 1 or 3, max_vals > 4096, n > 2^28, null pointers; n = 0
 * writes two zero counts and padded lists.
 * Scratch: the grow-only workspace the plookup shares, of
 *   zkgpu_multiset_diff_workspace_bytes(n) = 16 m + 16 n + 8 ceil(ceil(n / 1024) / 2) + 16 * 4097
 * bytes, m = the smallest power of two >= 4 n (0 for n = 0): a table of m slots x 4 u32 (the up
 * to 2 n distinct values at load <= 0.5), two n-row flag columns, the reduction's block counts
 * and the two row lists (host only, no GPU needed). */
uint64_t zkgpu_multiset_diff_workspace_bytes(uint64_t n);
int zkgpu_multiset_diff_dev(uint64_t *out, const uint64_t *a, uint64_t a_ld, const uint64_t *b, uint64_t b_ld,
                            uint64_t n, uint32_t dim, uint32_t max_vals);

/* The values of a plookup's source column f that no row of its table column t holds (the
 * prover's trace audit, include/zkgpu_stark.h zkgpu_stark_audit: calculateH1H2 stops at the first
 * such row, "Number not included"; this lists all of them).  Columns, values and dim as for
 * zkgpu_multiset_diff_dev: dim 1 or 3 with the components one leading dimension apart, a value is
 * the canonical dim-tuple (v and v + p are the same value).
 * out (device, 2 + 2 * max_vals words):
 *   out[0]  rows i < n of f whose value no row of t holds
 *   out[1]  distinct such values
 *   then max_vals pairs {the value's first row in f, its count in f}, ascending by that row;
 *   {UINT64_MAX, 0} past the last
 * One wrong value repeated on a million rows is ONE entry with count 1000000.
 * The result does not depend on the launch geometry or on which thread claims a table slot: the
 * table is the multiset difference's over f and t (counts are atomic sums, first rows atomic
 * minima), out[0] is the sum of the missing values' counts (added up per workgroup before one
 * atomic each), and the list comes from the reduction of zkgpu_nonzero_rows_dev over a flag on
 * each missing value's first row.  Enqueued on the library stream, no host synchronisation; rows
 * [n, ld) are not read; f == t is allowed.  ZKGPU_ERR_ARG, nothing queued: f_ld < n or t_ld < n,
 * dim not 1 or 3, max_vals > 4096, n > 2^28, null pointers; n = 0 writes two zero counts and a
 * padded list.
 * Scratch: the grow-only workspace of the plookup and the multiset difference, of
 *   zkgpu_lookup_misses_workspace_bytes(n) = 16 m + 8 n + 8 ceil(ceil(n / 1024) / 2) + 8 * 4097 + 8
 * bytes, m = the smallest power of two >= 4 n (0 for n = 0): the same table, one n-row flag
 * column, the reduction's block counts, one row list and the word out[0] adds up in -- never more
 * than zkgpu_multiset_diff_workspace_bytes(n), so one allocation serves both (host only, no GPU
 * needed). */
uint64_t zkgpu_lookup_misses_workspace_bytes(uint64_t n);
int zkgpu_lookup_misses_dev(uint64_t *out, const uint64_t *f, uint64_t f_ld, const uint64_t *t, uint64_t t_ld,
                            uint64_t n, uint32_t dim, uint32_t max_vals);

/* The cells that a connection check {a[0..k-1]} connect {S[0..k-1]} leaves unequal (the prover's
 * trace audit, include/zkgpu_stark.h zkgpu_stark_conn_check: the third answer beside
 * zkgpu_lookup_misses_dev and zkgpu_multiset_diff_dev).  On the trace domain of n = 2^n_bits rows
 * with generator w (the NTT's), cell (j, r) has the identity ks[j] w^r and the constant column
 * S_i holds at row r the identity of the cell that (i, r) is wired to; the grand product closes
 * exactly when S names every cell once and every cell holds the value of the cell it is wired to.
 * a and s are column-major sections with leading dimensions a_ld and s_ld; a_cols and s_cols
 * (host, k entries each, NULL: 0 .. k-1) list the k columns of each.  ks (host, k values, NULL:
 * 1, 12, 144, ... = 12^i) are the coset shifts.  ASSUMPTION: the default is pil-stark's getKs
 * with k = 12; a caller whose constants were built with other shifts passes them.
 * A cell is the number i n + r, i the index into the column lists.  out (device,
 * 3 + 6 * max_vals words):
 *   out[0]  broken cells: S_i[r] is the identity of a cell t and a(i, r) != a(t) mod p.  One
 *           wrong cell inside a cycle is two broken links, both naming it; a cell wired to itself
 *           never breaks
 *   out[1]  foreign cells: S_i[r] is no ks[j] w^r' (a damaged or mismatched constant file)
 *   out[2]  untargeted cells: no S value names them.  0 exactly when S, with no foreign cell, is a
 *           permutation of the cells
 *   then max_vals records {cell, target cell, value at cell, value at target} of the broken
 *   cells, ascending by cell, values canonical; {UINT64_MAX, 0, 0, 0} past the last
 *   then max_vals records {cell, S value} of the foreign cells; {UINT64_MAX, 0} past the last
 * None of this depends on a challenge.  Inputs may be non-canonical: v and v + p are one value,
 * S values too.  The result does not depend on the launch geometry: the target of an S value is
 * computed (v^n names the coset, the row comes out bit by bit in the subgroup of order 2^n_bits),
 * not looked up, every cell writes its own two flags, the marks of the named cells are idempotent
 * stores, the lists come from the reduction of zkgpu_nonzero_rows_dev over a flag per cell, and
 * out[2] is a sum added up per workgroup before one atomic each.  Enqueued on the library
 * stream, no host synchronisation; rows [n, ld) are not read.  ZKGPU_ERR_ARG, nothing queued (and
 * judged before the library's state, so a refusal needs no GPU): a_ld < n or s_ld < n, k = 0 or
 * k > 64, k n > 2^31, max_vals > 4096, n_bits > 28, a column repeated within a list, a zero in
 * ks or two cosets that collide ((ks[i] / ks[j])^n = 1, "the cosets of ks[i] and ks[j]
 * collide"), null pointers.
 * Scratch: the grow-only workspace of the plookup, of
 *   zkgpu_conn_breaks_workspace_bytes(n, k)
 *     = 16 c + 8 ceil(c / 2) + 8 ceil(ceil(c / 1024) / 2) + 16 * 4097 + 8,  c = k n
 * bytes: two flag columns of c u64, c u32 marks, the reduction's block counts, the two cell
 * lists and the word out[2] adds up in (host only, no GPU needed).
 * zkgpu_conn_ks_check judges k, n_bits and ks alone, with the same messages (host only). */
uint64_t zkgpu_conn_breaks_workspace_bytes(uint64_t n, uint32_t k);
int zkgpu_conn_ks_check(const uint64_t *ks, uint32_t k, uint32_t n_bits);
int zkgpu_conn_breaks_dev(uint64_t *out, const uint64_t *a, uint64_t a_ld, const uint32_t *a_cols, const uint64_t *s,
                          uint64_t s_ld, const uint32_t *s_cols, uint32_t k, const uint64_t *ks, uint32_t n_bits,
                          uint32_t max_vals);

/* 3 ext columns (ld >= n) -> interleaved n x 3 (the FRI polynomial layout, friProve.cpp) */
int zkgpu_cols3_to_interleaved_dev(uint64_t *out, const uint64_t *cols, uint64_t ld, uint64_t n);

/* MerkleTreeGL::getGroupProof for a row-major device source (FRI trees); the
 * same refusals as zkgpu_gl_merkle_open_dev */
int zkgpu_gl_merkle_open_rows_dev(uint64_t *vals_out, uint64_t *sibs_out, const uint64_t *nodes, const uint64_t *src,
                                  uint64_t ncols, uint64_t nrows, const uint64_t *idx, uint64_t nq);

/* The query phase's openings of several trees in one round trip
 * (friProve.cpp:195-232 -- every tree's getGroupProof at its query indices):
 * request k is zkgpu_gl_merkle_open_dev (rows = 0: src column-major, ld) or
 * zkgpu_gl_merkle_open_rows_dev (rows = 1: src row-major, ld ignored) with the
 * same arguments and output layout; one index upload, the n kernels, one
 * download, one synchronisation.  Every index is checked before anything is
 * queued. */
typedef struct zkgpu_open_req {
    uint64_t *vals_out, *sibs_out;
    const uint64_t *nodes, *src;
    uint64_t ld, ncols, nrows;
    const uint64_t *idx;
    uint64_t nq;
    uint32_t rows;
} zkgpu_open_req;
int zkgpu_gl_merkle_open_many(const zkgpu_open_req *req, uint32_t n);

/* ---- circom .exec hand-off -----------------------------------------------------
 * Circom*::getCommitedPols (main.recursive1.cpp:343-394, the same loop in main.cpp,
 * main.recursive2.cpp and main.recursiveF.cpp): from a circom witness to the committed
 * columns of C12a / recursive1 / recursive2 / recursiveF through the circuit's .exec file,
 *     tmp[0 .. size_witness)  = witness
 *     tmp[size_witness + i]   = tmp[idx_1] * c + tmp[idx_2] * d        add i = (idx_1, idx_2, c, d)
 *     column j, row i         = sMap[n_cols i + j] ? tmp[sMap[n_cols i + j]] : 0     (i < nSMap)
 *                               0                                                   (nSMap <= i < n)
 * image: the .exec file's u64 words [nAdds, nSMap, adds[4 nAdds], sMap[nSMap n_cols]]
 * (execFile.hpp:48-64).  sMap index 0 means "empty"; an add may read tmp[0].  Witness words and
 * coefficients are any u64 (reduced mod p); the columns are canonical.
 *
 * zkgpu_exec_create plans once per circuit, on the host (csrc/exec_plan.hpp): the adds are
 * levelled (an add's level is 1 + its operands' highest, witness slots 0) and sorted by level; a
 * level of more than 1024 adds is one grid launch, a run of consecutive narrower levels one
 * single-workgroup launch with a workgroup barrier between its levels; sMap is kept column-major
 * as u32.  The tables and the tmp buffer (size_witness + nAdds words) are uploaded / allocated in
 * one device block that lives in the handle.  The reference validates nothing; here ZKGPU_ERR_ARG
 * with a message naming the add or cell refuses: image_words != 2 + 4 nAdds + nSMap n_cols; an add
 * operand >= size_witness + i (a forward or self reference); an sMap entry >= size_witness +
 * nAdds; size_witness + nAdds >= 2^32 (slots are u32); n_cols == 0 or size_witness == 0.
 * zkgpu_exec_info: the counts, the schedule's depth, the kernel launches of one commit (the
 * segments and the gather) and the device block's bytes; any out pointer may be null.
 * zkgpu_exec_commit_dev: witness (host, size_witness words; free again when the call returns) ->
 * column j at cols + j * ld (device), rows [0, n) of every column written, zeros included, rows
 * [n, ld) untouched.  Queued on the library stream; the kernels are not waited for.  Refused:
 * n < nSMap, n > ld, null pointers.  One commit at a time per handle (tmp is the handle's).
 * zkgpu_exec_destroy waits for the library stream, then frees the block.
 * zkgpu_exec_set_tail_width: the widest level a single-workgroup launch takes, for the plans of
 * later zkgpu_exec_create calls (process-wide; 0: the default, 1024; above 1024: those calls are
 * refused).  The columns do not depend on it (tools/exec_commit_cost.py compares 256 and 1024).
 * There is no CPU path. */
void zkgpu_exec_set_tail_width(uint32_t max_adds);
int zkgpu_exec_create(void **exec, const uint64_t *image, uint64_t image_words, uint64_t size_witness,
                      uint32_t n_cols);
int zkgpu_exec_info(void *exec, uint64_t *n_adds, uint64_t *n_smap, uint32_t *n_levels, uint32_t *n_launches,
                    uint64_t *device_bytes);
int zkgpu_exec_commit_dev(void *exec, const uint64_t *witness, uint64_t *cols, uint64_t ld, uint64_t n);
void zkgpu_exec_destroy(void *exec);

/* ---- arithmetic self-test hook -----------------------------------------------
 * Runs one device field operation elementwise on arbitrary u64 inputs
 * (including non-canonical values >= p) and stores canonical results:
 * op 0 a+b, 1 a-b, 2 a*b, 3 -a, 4 a*2^12, 5 a*2^48, 6 a*2^84, 7 a*2^100,
 * 8 a^7, 9 cubic-extension a*b (a, b, out are n x 3).  Used by the parity
 * tests to pin the arithmetic core against big-integer references. */
int zkgpu_gl_field_selftest_dev(uint64_t *out, const uint64_t *a, const uint64_t *b, uint64_t n, int op);

/* The same for the helpers whose final correction runs behind a wave-uniform
 * branch (csrc/gl_rb.hpp; the NTT pass butterflies and the Poseidon S-box,
 * MDS and dot-product reductions use them), and every shift-multiply:
 * op 0 gl_add_rb(a, b), 1 gl_sub_rb(a, b), 2 gl_mul_rb(a, b),
 * 3 gl_reduce128_rb(lo = a, hi = b), 4 gl_reduce96_small_rb(lo = a, hl = b mod 2^32),
 * 5 dot3_fin_rb(A0 = a, A1 = b, A2 = c), 6 mul2e_rb<e>(a), 7 mul2e<e>(a) (0 <= e < 192),
 * 8 the Poseidon S-box a^7 (pow7), 9 its squaring gl_sqr3(a),
 * 10 gl_reduce128(lo = a, hi = b), 11 Dot3::fin(A0 = a, A1 = b, A2 = c),
 * 12 Dot2::fin(L = a, H = b), the two-accumulator reduction of the Poseidon
 * power blocks (a + 2^32 b; the kernels keep both below 2^58, the reduction is
 * exact for any a and any b < 2^63; it has no rare-branch variant: its
 * correction is common).
 * Canonical results; c is read by ops 5 and 11 only. */
int zkgpu_gl_field_selftest_rb_dev(uint64_t *out, const uint64_t *a, const uint64_t *b, const uint64_t *c, uint64_t n,
                                   int op, int e);

/* ---- live kernel profiling --------------------------------------------------
 * With profiling on, every kernel launch is bracketed by HIP events recorded
 * on the launch stream, tagged with the kernel name and its algorithmic bytes
 * (each input element read once, each output element written once).
 * zkgpu_prof_query synchronises the stream and returns, for one kernel name,
 * the launch count, summed device time (ms) and summed algorithmic bytes.
 * Replaces nothing in the reference (its TimerStart/TimerStopAndLog host
 * timers, starks.cpp:49-403, are kept by the host adapter). */
int zkgpu_prof_enable(int on);
int zkgpu_prof_reset(void);
int zkgpu_prof_query(const char *kernel, uint64_t *launches, double *total_ms, double *total_bytes);
/* names of kernels seen since the last reset, '\n'-separated, into buf */
int zkgpu_prof_kernels(char *buf, uint64_t buflen);

/* Stream marks (no reference counterpart: the reference times its stages on
 * the CPU, TimerStart / TimerStopAndLog around synchronous code): the host
 * prover's stage timers without a device synchronisation per stage.
 * zkgpu_mark records event `slot` (< ZKGPU_MARKS) on the library stream;
 * zkgpu_mark_elapsed waits for event b and returns the milliseconds from
 * event a to event b. */
#define ZKGPU_MARKS 256
int zkgpu_mark(uint32_t slot);
int zkgpu_mark_elapsed(uint32_t a, uint32_t b, double *ms);

#ifdef __cplusplus
}
#endif
#endif /* ZKGPU_H */
