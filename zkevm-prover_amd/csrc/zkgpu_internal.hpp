// Internal state of libzkgpu (not part of the C-ABI): the context and the
// launchers of the .hip files.  What needs no GPU is declared in headers
// without HIP, which the host-only sources and the stand-alone checks under
// tests/cpp include on their own: gl_host.hpp (the host field),
// zxp_jit_source.hpp (the expression kernels' source generator) and
// zxp_prepare.hpp (argument checks, plan and interpreter records of an
// expression evaluation).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/zkgpu.h"
#include "../../include/zkgpu_zxp.h"
#include "zxp_jit_source.hpp"  // ZxpJitIn, the host field (gl_host.hpp)
#include "zxp_prepare.hpp"     // ZOp, ZTerm, ZxpLaunch; ZxpArgs, ZxpPlan and the phases

namespace zk {

constexpr uint32_t NTT_MAX_PASSES = 4;  // log2 n <= 32 at radix <= 2^8
constexpr uint32_t POST_BITS = 12;  // LDE shift-power tables: lo 4096 entries

struct Workspace {
    void *ptr = nullptr;
    size_t bytes = 0;
};

struct Ctx {
    int device = -1;
    bool ready = false;
    hipStream_t stream = nullptr;  // launches go here (zkgpu_set_stream)
    // direction 0 = forward, 1 = inverse
    uint64_t *rt_small[2] = {nullptr, nullptr};  // omega_4096^k, k < 4096 (this direction)
    uint64_t *tw_lo[2] = {nullptr, nullptr};     // omega_{2^28}^i, i < 2^14
    uint64_t *tw_hi[2] = {nullptr, nullptr};     // omega_{2^28}^(2^14 i)
    // LDE post-scale tables (1/n * 7^k), cached per log n
    uint32_t post_logn = 0;
    uint64_t *post_lo = nullptr;
    uint64_t *post_hi = nullptr;
    // scratch workspaces
    Workspace ws[8];  // 0-3 NTT / staging, 4 H1H2 scratch, 5 rocPRIM temp, 6 ZXP segment carries,
                      // 7 nonzero-rows block counts
    // Poseidon constants on device
    uint64_t *poseidon_rc = nullptr;
};

Ctx &ctx();
int set_error(int code, const char *fmt, ...);
int check_launch(const char *what);
int check_hip(hipError_t e, const char *what);
// grow-only scratch buffer i
uint64_t *workspace(int i, size_t bytes);

// ---- live kernel profiling (HIP events on the launch stream; zkgpu_prof_*)
// prof_begin/prof_end bracket one kernel launch; bytes = algorithmic bytes
// (each input element read once + each output element written once).
bool prof_on();
void prof_begin(hipStream_t s);
void prof_end(const char *kernel, double bytes, hipStream_t s);

// ---- ntt.hip
int ntt_columns(Ctx &c, uint64_t *dst, uint64_t dst_ld, const uint64_t *src, uint64_t src_ld, uint64_t src_valid,
                uint64_t *tmp, uint64_t tmp_ld, uint32_t logn, uint64_t ncols, int inverse, const uint64_t *post_lo,
                const uint64_t *post_hi, uint32_t post_bits, uint64_t post_base, uint64_t post_scale, hipStream_t s);
void rows_to_cols(const uint64_t *in, uint64_t *out, uint64_t nrows, uint64_t ncols, uint64_t ld, hipStream_t s);
void cols_to_rows(const uint64_t *in, uint64_t *out, uint64_t nrows, uint64_t ncols, uint64_t ld, hipStream_t s);
void fill_powers(uint64_t *out, uint64_t base, uint64_t step, uint64_t scale, uint64_t count, hipStream_t s);
// 3-pass LDE 2^logn -> 2^(logn+1) (ntt.hip "3-pass LDE"); t1: 2^logn words per column
bool lde3_supported(uint32_t logn, uint32_t loge);
int lde3_columns(Ctx &c, uint64_t *out, uint64_t ld_out, const uint64_t *in, uint64_t ld_in, uint64_t *t1,
                 uint32_t logn, uint64_t ncols, hipStream_t s);

// ---- poseidon.hip
int poseidon_batch(uint64_t *out, const uint64_t *in, uint64_t n, int full, hipStream_t s);
int merkle_leaves_cols(uint64_t *digests, const uint64_t *src, uint64_t ncols, uint64_t nrows, uint64_t ld,
                       hipStream_t s, const uint64_t *src2 = nullptr, uint64_t split = 0);
int merkle_leaves_rows(uint64_t *digests, const uint64_t *src, uint64_t ncols, uint64_t nrows, hipStream_t s);
int merkle_levels(uint64_t *nodes, uint64_t nrows, hipStream_t s);
int merkle_open_cols(uint64_t *vals, uint64_t *sibs, const uint64_t *nodes, const uint64_t *src, uint64_t ncols,
                     uint64_t nrows, uint64_t ld, const uint64_t *idx, uint64_t nq, hipStream_t s);

// ---- h1h2.hip, row-sharded calculateH1H2 (host/sharded_starks.hpp)
int h1h2_shard_route(uint64_t *recs, uint64_t cap, uint32_t *n_t, uint32_t *n_f, const uint64_t *f, uint64_t f_ld,
                     const uint64_t *t, uint64_t t_ld, uint64_t n, uint64_t row0, uint32_t dim, uint32_t world,
                     hipStream_t s);
int h1h2_shard_owner(uint64_t *ret, const uint64_t *recs, uint64_t nrec, uint32_t dim, uint64_t *miss_row,
                     hipStream_t s);
int h1h2_shard_counts(uint32_t *start, uint32_t *cnt, uint64_t *total, const uint64_t *sent, const uint64_t *ret,
                      uint64_t nsent, uint64_t n, uint64_t row0, hipStream_t s);
int h1h2_shard_deal(uint64_t *seg, uint64_t seg_ld, const uint64_t *t, uint64_t t_ld, const uint32_t *start,
                    const uint32_t *cnt, uint64_t n, uint32_t dim, hipStream_t s);
int h1h2_shard_place(uint64_t *h1, uint64_t h1_ld, uint64_t *h2, uint64_t h2_ld, const uint64_t *buf, uint64_t buf_ld,
                     uint64_t pos0, uint64_t len, uint64_t row0, uint32_t dim, hipStream_t s);

// ---- fri.hip
int fri_fold(uint64_t *out, const uint64_t *pol, uint32_t pol_bits, uint32_t out_bits, const uint64_t sx[3],
             uint64_t shift_inv, hipStream_t s);
int fri_fold_rows(uint64_t *out, const uint64_t *rows, uint64_t g0, uint64_t n_local, uint32_t pol_bits,
                  uint32_t out_bits, const uint64_t sx[3], uint64_t shift_inv, hipStream_t s);
int fri_transpose(uint64_t *aux, const uint64_t *pol, uint64_t degree, uint32_t tbits, hipStream_t s);

// ---- zxp_jit.hip: run-time compiled straight-line expression kernels
// (ZxpJitIn: csrc/zxp_jit_source.hpp)
// 0 launched, 1 shape unsupported (run the interpreter), < 0 error
int zxp_jit_run(const ZxpJitIn &in, hipStream_t s);

// ---- stark.hip
// (the interpreter's records ZOp / ZTerm and its launch ZxpLaunch: csrc/zxp_prepare.hpp)
int rand_cols(uint64_t *base, uint64_t ld, const uint32_t *cols_dev, uint32_t ncols, uint64_t nrows, uint64_t seed,
              uint64_t stream, uint64_t row0, uint64_t rmask, hipStream_t s);
int copy_rows(uint64_t *dst, uint64_t dld, uint64_t drow0, const uint32_t *dcols, const uint64_t *src, uint64_t sld,
              uint64_t srow0, uint64_t smask, const uint32_t *scols, uint32_t ncols, uint64_t nrows, hipStream_t s);
int zxp_eval(const ZxpLaunch &L, hipStream_t s);
// the same at the rows rows[0 .. n_rows) (device), stores compact (k_zxp_eval_rows)
int zxp_eval_rows(const ZxpLaunch &L, const uint64_t *rows, uint32_t n_rows, hipStream_t s);
// the nonzero rows of a column-major section (k_nz_count / k_nz_emit): out = 1 + max_rows words,
// counts = nonzero_rows_blocks(n) words of device scratch
uint32_t nonzero_rows_blocks(uint64_t n);
int nonzero_rows(uint64_t *out, uint32_t *counts, const uint64_t *cols, uint64_t ld, uint32_t ncols, uint64_t n,
                 uint32_t max_rows, hipStream_t s);
size_t calculate_z_scratch_words(uint64_t n);
int calculate_z(uint64_t *z, uint64_t z_ld, const uint64_t *num, uint64_t num_ld, const uint64_t *den,
                uint64_t den_ld, uint64_t n, const uint64_t z0[3], uint64_t *scratch, uint64_t *total_dev, hipStream_t s);
size_t evmap_group_size();
uint32_t evmap_group_width();
uint64_t evmap_rows_per_block();
int evmap_groups(uint64_t *evals, const void *groups_dev, uint32_t n_groups, uint32_t width, uint32_t unroll,
                 const int32_t *subs_dev,
                 uint32_t n_ev, uint32_t n_sub, const uint64_t *lev, const uint64_t *lpev, uint64_t l_ld, uint64_t n, uint32_t eb,
                 uint64_t *partial, hipStream_t s);
int xdivxsub(uint64_t *xdiv, uint64_t *xdivw, const uint64_t xi[3], uint64_t w, uint32_t logn, hipStream_t s);
int xdivxsub_rows(uint64_t *xdiv, uint64_t *xdivw, const uint64_t xi[3], uint64_t w, uint32_t logn, uint64_t row0,
                  uint64_t nrows, hipStream_t s);
int xdiv_rows(uint64_t *out0, uint64_t *out1, uint64_t ld, int interleaved, const uint64_t a0[3],
              const uint64_t a1[3], uint64_t shift, const uint64_t scale[3], uint32_t logn, uint64_t row0,
              uint64_t nrows, hipStream_t s);
int ext_powers(uint64_t *out, uint64_t ld, const uint64_t base[3], uint64_t n, hipStream_t s);
int scale_powers(uint64_t *cols, uint64_t ld, uint32_t ncols, uint64_t n, uint64_t base, hipStream_t s);
int qsplit(uint64_t *qq2, uint64_t ld2, const uint64_t *qq1, uint64_t ld1, uint64_t n, uint32_t qdeg,
           uint64_t shift_in, uint32_t dim, uint32_t stride, hipStream_t s);
int cols3_to_interleaved(uint64_t *out, const uint64_t *cols, uint64_t ld, uint64_t n, hipStream_t s);
int h1h2(uint64_t *h1, uint64_t h1_ld, uint64_t *h2, uint64_t h2_ld, const uint64_t *f, uint64_t f_ld,
         const uint64_t *t, uint64_t t_ld, uint64_t n, uint32_t dim, uint64_t *missing_row, hipStream_t s);
// the distinct values of two columns whose multiplicities differ (h1h2.hip "multiset difference")
uint64_t multiset_diff_workspace_bytes(uint64_t n);
int multiset_diff(uint64_t *out, const uint64_t *a, uint64_t a_ld, const uint64_t *b, uint64_t b_ld, uint64_t n,
                  uint32_t dim, uint32_t max_vals, hipStream_t s);
int merkle_open_strided(uint64_t *vals, uint64_t *sibs, const uint64_t *nodes, const uint64_t *src, uint64_t ncols,
                        uint64_t nrows, uint64_t row_stride, uint64_t col_stride, const uint64_t *idx, uint64_t nq,
                        hipStream_t s);

}  // namespace zk
