// The cells a connection check {a[0..k-1]} connect {S[0..k-1]} leaves unequal
// (the prover's trace audit; include/zkgpu.h zkgpu_conn_breaks_dev).  Cell
// (j, r) of the n = 2^n_bits row trace has the identity ks[j] w^r, and S_i[r]
// holds the identity of the cell that (i, r) is wired to.
//
// No table: the target of an S value v is found by arithmetic alone.
//   column  v = ks[j] w^r  =>  v^n = ks[j]^n, and the ks[j]^n are distinct
//           exactly when the cosets are (the refusal of colliding ks below):
//           n_bits squarings and k compares name j, or no j -- a foreign value
//   row     u = v / ks[j] lies in the subgroup of order 2^n_bits, so r comes
//           out bit by bit (Pohlig-Hellman): bit b of r is set iff
//           (u w^-(r mod 2^b))^(2^(n_bits-1-b)) = -1; n_bits (n_bits - 1) / 2
//           squarings and at most n_bits products by the w^-(2^b) of the
//           kernel's arguments
// That is ~275 field products per cell at 2^22 rows and no memory traffic
// beyond the two columns, against one random access per cell into a table of
// 2 k n keyed identities (DESIGN.md "Connection breaks").  Every thread owns
// its cell: the two flag columns hold 0 or 1 per cell whatever the launch
// geometry, the "named" marks are idempotent stores, the lists come from the
// nonzero-rows reduction (stark.hip) and the untargeted count is a sum of
// integers added up per workgroup before one atomic each.
#include <algorithm>

#include "gl_device.hpp"
#include "gl_host.hpp"
#include "zkgpu_internal.hpp"

namespace zk {

constexpr uint32_t CONN_MAX_COLS = 64;
constexpr uint32_t CONN_MAX_BITS = 28;
constexpr uint32_t CONN_MAX_VALS = 4096;    // = NZ_MAX_ROWS (the lists come from k_nz_emit)
constexpr uint32_t CONN_COUNT_BLOCKS = 1024;  // grid-stride cap of k_conn_count
constexpr uint32_t CONN_NONE = 0xFFFFFFFFu;

static inline uint32_t nblk3(uint64_t n, uint32_t t) { return (uint32_t)((n + t - 1) / t); }

struct ConnArgs {
    const uint64_t *a, *s;
    uint64_t a_ld, s_ld, n;
    uint32_t k, n_bits;
    uint32_t acol[CONN_MAX_COLS], scol[CONN_MAX_COLS];
    uint64_t ksn[CONN_MAX_COLS];    // ks[j]^n, canonical
    uint64_t ksinv[CONN_MAX_COLS];  // 1 / ks[j]
    uint64_t winv[CONN_MAX_BITS];   // w^-(2^b)
};

// the cell j n + r whose identity is the canonical value v, CONN_NONE if v is no ks[j] w^r
__device__ __forceinline__ uint32_t conn_target(const ConnArgs &A, uint64_t v)
{
    uint64_t y = v;
    for (uint32_t b = 0; b < A.n_bits; b++) y = gl_sqr(y);
    y = gl_canon(y);
    uint32_t j = CONN_NONE;
    for (uint32_t c = 0; c < A.k; c++)
        if (A.ksn[c] == y) j = c;  // (at most one: the ks[c]^n are distinct)
    if (j == CONN_NONE) return CONN_NONE;
    uint64_t g = gl_mul(v, A.ksinv[j]);  // of order dividing 2^n_bits
    uint32_t r = 0;
    for (uint32_t b = 0; b < A.n_bits; b++) {
        uint64_t t = g;
        for (uint32_t q = b + 1; q < A.n_bits; q++) t = gl_sqr(t);
        if (gl_canon(t) != 1) {  // = -1: bit b of r
            r |= 1u << b;
            g = gl_mul(g, A.winv[b]);
        }
    }
    return gl_canon(g) == 1 ? j * (uint32_t)A.n + r : CONN_NONE;
}

__device__ __forceinline__ uint64_t conn_a(const ConnArgs &A, uint32_t cell)
{
    const uint32_t i = cell >> A.n_bits;
    return gl_canon(A.a[(uint64_t)A.acol[i] * A.a_ld + (cell & (uint32_t)(A.n - 1))]);
}

__device__ __forceinline__ uint64_t conn_s(const ConnArgs &A, uint32_t cell)
{
    const uint32_t i = cell >> A.n_bits;
    return gl_canon(A.s[(uint64_t)A.scol[i] * A.s_ld + (cell & (uint32_t)(A.n - 1))]);
}

// cell g: its two flags, and the mark on the cell it names
__global__ void __launch_bounds__(256) k_conn_probe(uint64_t *broken, uint64_t *foreign, uint32_t *named, ConnArgs A)
{
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (uint64_t)A.k * A.n) return;
    const uint32_t t = conn_target(A, conn_s(A, (uint32_t)g));
    uint64_t br = 0;
    if (t != CONN_NONE) {
        named[t] = 1;
        br = conn_a(A, (uint32_t)g) != conn_a(A, t);
    }
    broken[g] = br;
    foreign[g] = t == CONN_NONE;
}

// the cells that no S value names
__global__ void __launch_bounds__(256) k_conn_count(unsigned long long *n_untargeted, const uint32_t *named,
                                                    uint64_t cells)
{
    __shared__ uint32_t part[4];
    uint32_t sum = 0;  // cells <= 2^31
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < cells; c += stride) sum += named[c] == 0;
#pragma unroll
    for (int off = 32; off; off >>= 1) sum += (uint32_t)__shfl_down((int)sum, off);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t tot = part[0] + part[1] + part[2] + part[3];
        if (tot) atomicAdd(n_untargeted, (unsigned long long)tot);
    }
}

// out = {3 counts, max_vals x {cell, target, a(cell), a(target)}, max_vals x {cell, S value}}
__global__ void __launch_bounds__(256) k_conn_emit(uint64_t *out, const uint64_t *listb, const uint64_t *listf,
                                                   const unsigned long long *n_untargeted, uint32_t max_vals,
                                                   ConnArgs A)
{
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e == 0) {
        out[0] = listb[0];
        out[1] = listf[0];
        out[2] = *n_untargeted;
    }
    if (e >= max_vals) return;
    const uint64_t cells = (uint64_t)A.k * A.n;
    uint64_t *ob = out + 3 + 4ULL * e, *of = out + 3 + 4ULL * max_vals + 2ULL * e;
    const uint64_t cb = listb[1 + e], cf = listf[1 + e];  // (the reduction pads its lists with UINT64_MAX)
    uint64_t tgt = 0, va = 0, vt = 0, sv = 0;
    if (cb < cells) {
        const uint32_t t = conn_target(A, conn_s(A, (uint32_t)cb));  // a listed cell has one
        tgt = t;
        va = conn_a(A, (uint32_t)cb);
        vt = t != CONN_NONE ? conn_a(A, t) : 0;
    }
    if (cf < cells) sv = conn_s(A, (uint32_t)cf);
    ob[0] = cb < cells ? cb : UINT64_MAX;
    ob[1] = tgt;
    ob[2] = va;
    ob[3] = vt;
    of[0] = cf < cells ? cf : UINT64_MAX;
    of[1] = sv;
}

// the layout of the workspace (include/zkgpu.h states the sum)
struct ConnLayout {
    uint64_t broken, foreign, named, counts, lists, sum, total;
};
static ConnLayout conn_layout(uint64_t cells)
{
    ConnLayout L;
    L.broken = 0;                                                     // two flag columns of cells u64
    L.foreign = L.broken + 8 * cells;
    L.named = L.foreign + 8 * cells;                                  // cells u32
    L.counts = L.named + 8 * ((cells + 1) / 2);                       // the nonzero-rows block counts
    L.lists = L.counts + 8 * (((uint64_t)nonzero_rows_blocks(cells) + 1) / 2);  // 2 lists of 1 + CONN_MAX_VALS u64
    L.sum = L.lists + 2 * 8 * (1 + (uint64_t)CONN_MAX_VALS);
    L.total = L.sum + 8;
    return L;
}

uint64_t conn_breaks_workspace_bytes(uint64_t n, uint32_t k) { return conn_layout(n * k).total; }

// the default ks: 1, 12, 144, ... (pil-stark's getKs with k = 12, an assumption include/zkgpu.h states)
static void conn_default_ks(uint64_t *ks, uint32_t k)
{
    ks[0] = 1;
    for (uint32_t i = 1; i < k; i++) ks[i] = h_mul(ks[i - 1], 12);
}

// 0, or the refusal: ksn = ks[j]^n on return
static int conn_check_ks(uint64_t *ksn, const uint64_t *ks, uint32_t k, uint32_t n_bits)
{
    for (uint32_t j = 0; j < k; j++) {
        if (ks[j] % HP == 0) return set_error(ZKGPU_ERR_ARG, "conn_breaks: ks[%u] is zero", j);
        ksn[j] = h_pow(ks[j], 1ULL << n_bits);
        for (uint32_t i = 0; i < j; i++)
            if (ksn[i] == ksn[j])
                return set_error(ZKGPU_ERR_ARG, "conn_breaks: the cosets of ks[%u] and ks[%u] collide", i, j);
    }
    return 0;
}

static int conn_check_cols(uint32_t *dst, const uint32_t *cols, uint32_t k, const char *which)
{
    for (uint32_t i = 0; i < k; i++) {
        dst[i] = cols ? cols[i] : i;
        for (uint32_t j = 0; j < i; j++)
            if (dst[j] == dst[i])
                return set_error(ZKGPU_ERR_ARG, "conn_breaks: column %u repeated in %s", dst[i], which);
    }
    return 0;
}

// the arguments' checks (no GPU needed): A filled on success
static int conn_args(ConnArgs &A, const uint64_t *a, uint64_t a_ld, const uint32_t *a_cols, const uint64_t *s,
                     uint64_t s_ld, const uint32_t *s_cols, uint32_t k, const uint64_t *ks, uint32_t n_bits,
                     uint32_t max_vals)
{
    if (k == 0 || k > CONN_MAX_COLS)
        return set_error(ZKGPU_ERR_ARG, "conn_breaks: k = %u not in 1 .. %u", k, CONN_MAX_COLS);
    if (n_bits > CONN_MAX_BITS) return set_error(ZKGPU_ERR_ARG, "conn_breaks: more than 2^28 rows");
    const uint64_t n = 1ULL << n_bits;
    if ((uint64_t)k * n > (1ULL << 31)) return set_error(ZKGPU_ERR_ARG, "conn_breaks: more than 2^31 cells");
    if (max_vals > CONN_MAX_VALS)
        return set_error(ZKGPU_ERR_ARG, "conn_breaks: max_vals %u > %u", max_vals, CONN_MAX_VALS);
    if (a_ld < n || s_ld < n) return set_error(ZKGPU_ERR_ARG, "conn_breaks: ld < n");
    int rc;
    if ((rc = conn_check_cols(A.acol, a_cols, k, "a_cols")) || (rc = conn_check_cols(A.scol, s_cols, k, "s_cols")))
        return rc;
    uint64_t dks[CONN_MAX_COLS];
    if (!ks) {
        conn_default_ks(dks, k);
        ks = dks;
    }
    if ((rc = conn_check_ks(A.ksn, ks, k, n_bits))) return rc;
    for (uint32_t j = 0; j < k; j++) A.ksinv[j] = h_inv(ks[j] % HP);
    uint64_t wi = h_inv(h_w(n_bits));
    for (uint32_t b = 0; b < n_bits; b++, wi = h_mul(wi, wi)) A.winv[b] = wi;
    A.a = a, A.s = s, A.a_ld = a_ld, A.s_ld = s_ld, A.n = n, A.k = k, A.n_bits = n_bits;
    return 0;
}

static int conn_breaks(uint64_t *out, const ConnArgs &A, uint32_t max_vals, hipStream_t s)
{
    const uint64_t cells = (uint64_t)A.k * A.n;
    const ConnLayout L = conn_layout(cells);
    char *w = (char *)workspace(4, L.total);
    if (!w) return ZKGPU_ERR_OOM;
    uint64_t *broken = (uint64_t *)(w + L.broken), *foreign = (uint64_t *)(w + L.foreign);
    uint32_t *named = (uint32_t *)(w + L.named), *counts = (uint32_t *)(w + L.counts);
    uint64_t *listb = (uint64_t *)(w + L.lists), *listf = listb + 1 + CONN_MAX_VALS;
    unsigned long long *sum = (unsigned long long *)(w + L.sum);
    const uint32_t B = 256;
    // no cell named yet, the count zero (the probe writes both flags of every cell)
    if (check_hip(hipMemsetAsync(named, 0, 4 * cells, s), "conn_breaks memset") ||
        check_hip(hipMemsetAsync(sum, 0, 8, s), "conn_breaks memset"))
        return ZKGPU_ERR_HIP;
    prof_begin(s);
    hipLaunchKernelGGL(k_conn_probe, dim3(nblk3(cells, B)), dim3(B), 0, s, broken, foreign, named, A);
    prof_end("k_conn_probe", 36.0 * (double)cells, s);
    prof_begin(s);
    hipLaunchKernelGGL(k_conn_count, dim3(std::min(nblk3(cells, B), CONN_COUNT_BLOCKS)), dim3(B), 0, s, sum, named,
                       cells);
    prof_end("k_conn_count", 4.0 * (double)cells, s);
    if (check_launch("conn_breaks")) return ZKGPU_ERR_HIP;
    int rc;
    if ((rc = nonzero_rows(listb, counts, broken, cells, 1, cells, max_vals, s)) ||
        (rc = nonzero_rows(listf, counts, foreign, cells, 1, cells, max_vals, s)))
        return rc;
    prof_begin(s);
    hipLaunchKernelGGL(k_conn_emit, dim3(nblk3(max_vals ? max_vals : 1, B)), dim3(B), 0, s, out, listb, listf, sum,
                       max_vals, A);
    prof_end("k_conn_emit", 8.0 * (3 + 6.0 * max_vals), s);
    return check_launch("conn_breaks");
}

}  // namespace zk

// the C-ABI of the connection breaks (include/zkgpu.h), beside its kernels
extern "C" uint64_t zkgpu_conn_breaks_workspace_bytes(uint64_t n, uint32_t k)
{
    return zk::conn_breaks_workspace_bytes(n, k);
}

extern "C" int zkgpu_conn_ks_check(const uint64_t *ks, uint32_t k, uint32_t n_bits)
{
    if (k == 0 || k > zk::CONN_MAX_COLS)
        return zk::set_error(ZKGPU_ERR_ARG, "conn_breaks: k = %u not in 1 .. %u", k, zk::CONN_MAX_COLS);
    if (n_bits > zk::CONN_MAX_BITS) return zk::set_error(ZKGPU_ERR_ARG, "conn_breaks: more than 2^28 rows");
    uint64_t dks[zk::CONN_MAX_COLS], ksn[zk::CONN_MAX_COLS];
    if (!ks) {
        zk::conn_default_ks(dks, k);
        ks = dks;
    }
    return zk::conn_check_ks(ksn, ks, k, n_bits);
}

extern "C" int zkgpu_conn_breaks_dev(uint64_t *out, const uint64_t *a, uint64_t a_ld, const uint32_t *a_cols,
                                     const uint64_t *s, uint64_t s_ld, const uint32_t *s_cols, uint32_t k,
                                     const uint64_t *ks, uint32_t n_bits, uint32_t max_vals)
{
    if (!out || !a || !s) return zk::set_error(ZKGPU_ERR_ARG, "conn_breaks: null pointer");
    // the arguments are judged before the library's state: a refusal needs no GPU
    zk::ConnArgs A;
    int rc;
    if ((rc = zk::conn_args(A, a, a_ld, a_cols, s, s_ld, s_cols, k, ks, n_bits, max_vals))) return rc;
    if (!zk::ctx().ready) return zk::set_error(ZKGPU_ERR_INIT, "zkgpu_init() not called");
    return zk::conn_breaks(out, A, max_vals, zk::ctx().stream);
}
