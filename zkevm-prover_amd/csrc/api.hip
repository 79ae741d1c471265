// libzkgpu C-ABI (include/zkgpu.h): context, tables, host-pointer drop-ins
// and device-resident entry points.  All bulk arithmetic runs in the HIP
// kernels of ntt.hip / poseidon.hip / fri.hip; the host only stages buffers
// and computes a handful of scalar constants (roots, inverses).
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <deque>
#include <map>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

#include "gl_device.hpp"
#include "zkgpu_internal.hpp"
#include "poseidon_gl_constants.h"
#include "poseidon_gl_sparse.h"

namespace zk {

int upload_poseidon_constants(Ctx &c);
// poseidon.hip: one chunk of the chunked leaf sponge (k_leaves_absorb)
int merkle_leaves_absorb(uint64_t *nodes, const uint64_t *src, uint64_t ld, uint64_t col0, uint64_t ncols,
                         uint64_t total, uint64_t nrows, hipStream_t s);

static Ctx g_ctx;
static thread_local char g_err[512] = "";

Ctx &ctx() { return g_ctx; }

int set_error(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

int check_hip(hipError_t e, const char *what)
{
    if (e != hipSuccess) return set_error(ZKGPU_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
    return ZKGPU_OK;
}

int check_launch(const char *what) { return check_hip(hipGetLastError(), what); }

uint64_t *workspace(int i, size_t bytes)
{
    Workspace &w = g_ctx.ws[i];
    if (w.bytes >= bytes) return (uint64_t *)w.ptr;
    if (w.ptr) {
        (void)hipStreamSynchronize(g_ctx.stream);
        (void)hipFree(w.ptr);
        w.ptr = nullptr;
        w.bytes = 0;
    }
    if (hipMalloc(&w.ptr, bytes) != hipSuccess) {
        w.ptr = nullptr;
        set_error(ZKGPU_ERR_OOM, "workspace %d: hipMalloc(%zu) failed", i, bytes);
        return nullptr;
    }
    w.bytes = bytes;
    return (uint64_t *)w.ptr;
}

// ---- host scalar field: csrc/gl_host.cpp
static int alloc_dev(uint64_t **p, size_t n)
{
    if (hipMalloc((void **)p, n * sizeof(uint64_t)) != hipSuccess)
        return set_error(ZKGPU_ERR_OOM, "hipMalloc(%zu) failed", n * sizeof(uint64_t));
    return 0;
}

// LDE post-scale tables: factor(k) = 1/n * 7^k = lo[k & 4095] * hi[k >> 12]
static int ensure_post_tables(uint32_t logn)
{
    Ctx &c = g_ctx;
    if (c.post_lo && c.post_logn == logn) return 0;
    if (c.post_lo) {
        (void)hipStreamSynchronize(c.stream);
        (void)hipFree(c.post_lo);
        (void)hipFree(c.post_hi);
        c.post_lo = c.post_hi = nullptr;
    }
    uint64_t n = 1ULL << logn;
    uint64_t nlo = 1ULL << POST_BITS;
    uint64_t nhi = n > nlo ? n >> POST_BITS : 1;
    int rc;
    if ((rc = alloc_dev(&c.post_lo, nlo)) || (rc = alloc_dev(&c.post_hi, nhi))) return rc;
    fill_powers(c.post_lo, 7, 1, 1, nlo, c.stream);
    fill_powers(c.post_hi, 7, nlo, h_inv(n), nhi, c.stream);
    c.post_logn = logn;
    return check_launch("post tables");
}

static int require_init()
{
    if (!g_ctx.ready) return set_error(ZKGPU_ERR_INIT, "zkgpu_init() not called");
    return 0;
}

static bool is_pow2(uint64_t n) { return n && !(n & (n - 1)); }
static uint32_t log2u(uint64_t n)
{
    uint32_t l = 0;
    while ((1ULL << l) < n) l++;
    return l;
}

// Columns per extend_pol batch: the batch's coefficients (n words per
// column) and, on the 6-pass path, its 2n-row scratch live in grow-only
// workspaces, so the batch bounds that memory -- 2^31 words (16 GiB) of
// scratch.  (Batches of 32 columns
// at 2^24 rows measured 2-3 % slower than one batch of 100: 51.9 vs 53.5
// Gelem/s, the same box.)
static uint64_t g_lde_batch_max = 0;  // zkgpu_set_lde_batch_cols (0: the default)
static uint64_t lde_batch_cols(uint64_t n_ext, uint64_t ncols)
{
    uint64_t batch = std::max<uint64_t>(1, (1ULL << 31) / (n_ext ? n_ext : 1));
    if (g_lde_batch_max && g_lde_batch_max < batch) batch = g_lde_batch_max;
    return batch < ncols ? batch : ncols;
}

static uint64_t lde_workspace_bytes(uint64_t n, uint64_t n_ext, uint64_t ncols)
{
    const uint64_t b = lde_batch_cols(n_ext, ncols);
    return b * n * 8 + (lde3_supported(log2u(n), log2u(n_ext)) ? 0 : b * n_ext * 8);
}

// device LDE on column-major buffers
static int extend_pol_dev(uint64_t *out, uint64_t ld_out, const uint64_t *in, uint64_t ld_in, uint64_t n_ext,
                          uint64_t n, uint64_t ncols)
{
    if (!ncols || !n) return 0;
    if (!is_pow2(n) || !is_pow2(n_ext) || n_ext < n)
        return set_error(ZKGPU_ERR_ARG, "extend_pol: sizes must be powers of two with n_ext >= n");
    uint32_t logn = log2u(n), loge = log2u(n_ext);
    if (loge > TW_MAX_LOG) return set_error(ZKGPU_ERR_ARG, "extend_pol: n_ext > 2^%u", TW_MAX_LOG);
    int rc;
    if ((rc = ensure_post_tables(logn))) return rc;
    Ctx &c = g_ctx;
    const uint64_t batch = lde_batch_cols(n_ext, ncols);
    uint64_t *coef = workspace(0, batch * n * sizeof(uint64_t));
    if (!coef) return ZKGPU_ERR_OOM;
    if (lde3_supported(logn, loge)) {
        for (uint64_t c0 = 0; c0 < ncols; c0 += batch) {
            const uint64_t nc = ncols - c0 < batch ? ncols - c0 : batch;
            if ((rc = lde3_columns(c, out + c0 * ld_out, ld_out, in + c0 * ld_in, ld_in, coef, logn, nc, c.stream)))
                return rc;
        }
        return 0;
    }
    uint64_t *tmp = workspace(1, batch * n_ext * sizeof(uint64_t));
    if (!tmp) return ZKGPU_ERR_OOM;
    uint32_t post_bits = logn < POST_BITS ? logn : POST_BITS;
    for (uint64_t c0 = 0; c0 < ncols; c0 += batch) {
        uint64_t nc = ncols - c0 < batch ? ncols - c0 : batch;
        // coefficients * 7^k / n
        if ((rc = ntt_columns(c, coef, n, in + c0 * ld_in, ld_in, n, tmp, n, logn, nc, 1, c.post_lo, c.post_hi,
                              post_bits, 7, 1, c.stream)))
            return rc;
        // evaluations on the extended domain (zero padding = predicated loads)
        if ((rc = ntt_columns(c, out + c0 * ld_out, ld_out, coef, n, n, tmp, n_ext, loge, nc, 0, nullptr, nullptr, 0,
                              1, 1, c.stream)))
            return rc;
    }
    return 0;
}

static int ntt_dev(uint64_t *dst, uint64_t ld_dst, const uint64_t *src, uint64_t ld_src, uint64_t n, uint64_t ncols,
                   int inverse)
{
    if (!ncols || !n) return 0;
    if (!is_pow2(n)) return set_error(ZKGPU_ERR_ARG, "ntt: n must be a power of two");
    uint32_t logn = log2u(n);
    if (logn > TW_MAX_LOG) return set_error(ZKGPU_ERR_ARG, "ntt: n > 2^%u", TW_MAX_LOG);
    Ctx &c = g_ctx;
    uint64_t *tmp = nullptr;
    if (logn > 12) {
        tmp = workspace(1, ncols * n * sizeof(uint64_t));
        if (!tmp) return ZKGPU_ERR_OOM;
    }
    uint64_t scale = inverse ? h_inv(n) : 1;
    return ntt_columns(c, dst, ld_dst, src, ld_src, n, tmp, n, logn, ncols, inverse, nullptr, nullptr, 0, 1, scale,
                       c.stream);
}

__global__ void k_field_selftest(uint64_t *out, const uint64_t *a, const uint64_t *b, uint64_t n, int op)
{
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (op == 9) {
        gl3 x{{a[3 * i], a[3 * i + 1], a[3 * i + 2]}}, y{{b[3 * i], b[3 * i + 1], b[3 * i + 2]}};
        gl3 r = gl3_canon(gl3_mul(x, y));
        out[3 * i] = r.v[0];
        out[3 * i + 1] = r.v[1];
        out[3 * i + 2] = r.v[2];
        return;
    }
    uint64_t x = a[i], y = b[i], r = 0;
    switch (op) {
    case 0: r = gl_add(x, y); break;
    case 1: r = gl_sub(x, y); break;
    case 2: r = gl_mul(x, y); break;
    case 3: r = gl_neg(x); break;
    case 4: r = mul2e<12>(x); break;
    case 5: r = mul2e<48>(x); break;
    case 6: r = mul2e<84>(x); break;
    case 7: r = mul2e<100>(x); break;
    case 8: {
        uint64_t x2 = gl_mul(x, x), x3 = gl_mul(x2, x), x4 = gl_mul(x2, x2);
        r = gl_mul(x3, x4);
        break;
    }
    default: break;
    }
    out[i] = gl_canon(r);
}

}  // namespace zk

using namespace zk;

extern "C" {

int zkgpu_gl_field_selftest_dev(uint64_t *out, const uint64_t *a, const uint64_t *b, uint64_t n, int op)
{
    int rc;
    if ((rc = require_init())) return rc;
    if (op < 0 || op > 9) return set_error(ZKGPU_ERR_ARG, "field_selftest: unknown op %d", op);
    if (!n) return 0;
    hipLaunchKernelGGL(k_field_selftest, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, g_ctx.stream, out, a, b, n,
                       op);
    return check_launch("k_field_selftest");
}

int zkgpu_abi_version(void) { return 1; }

const char *zkgpu_last_error(void) { return g_err; }

int zkgpu_init(int device)
{
    Ctx &c = g_ctx;
    if (device < 0) {
        // keep whatever is initialised / current (torch.cuda.set_device in a rank)
        if (c.ready) return 0;
        int cur = 0;
        if (hipGetDevice(&cur) != hipSuccess) cur = 0;
        device = cur;
    }
    if (c.ready && c.device == device) return 0;
    if (c.ready) zkgpu_release();
    int rc;
    if ((rc = check_hip(hipSetDevice(device), "hipSetDevice"))) return rc;
    c.device = device;
    for (int d = 0; d < 2; d++) {
        if ((rc = alloc_dev(&c.rt_small[d], 4096)) || (rc = alloc_dev(&c.tw_lo[d], TW_LEVEL_SIZE)) ||
            (rc = alloc_dev(&c.tw_hi[d], TW_LEVEL_SIZE)))
            return rc;
        uint64_t w12 = h_w(12), w28 = h_w(TW_MAX_LOG);
        if (d) {
            w12 = h_inv(w12);
            w28 = h_inv(w28);
        }
        fill_powers(c.rt_small[d], w12, 1, 1, 4096, c.stream);
        fill_powers(c.tw_lo[d], w28, 1, 1, TW_LEVEL_SIZE, c.stream);
        fill_powers(c.tw_hi[d], w28, TW_LEVEL_SIZE, 1, TW_LEVEL_SIZE, c.stream);
    }
    if ((rc = upload_poseidon_constants(c))) return rc;
    if ((rc = check_launch("init tables"))) return rc;
    if ((rc = check_hip(hipStreamSynchronize(c.stream), "init sync"))) return rc;
    c.ready = true;
    return 0;
}

void zkgpu_release(void)
{
    Ctx &c = g_ctx;
    if (!c.ready) return;
    (void)hipDeviceSynchronize();
    for (int d = 0; d < 2; d++) {
        (void)hipFree(c.rt_small[d]);
        (void)hipFree(c.tw_lo[d]);
        (void)hipFree(c.tw_hi[d]);
    }
    if (c.post_lo) (void)hipFree(c.post_lo);
    if (c.post_hi) (void)hipFree(c.post_hi);
    for (auto &w : c.ws)
        if (w.ptr) (void)hipFree(w.ptr);
    c = Ctx();
}

int zkgpu_set_stream(void *s)
{
    g_ctx.stream = (hipStream_t)s;
    return 0;
}

void *zkgpu_get_stream(void) { return (void *)g_ctx.stream; }

int zkgpu_synchronize(void) { return check_hip(hipStreamSynchronize(g_ctx.stream), "synchronize"); }

// ---------------------------------------------------------------- NTT
int zkgpu_gl_ntt_dev(uint64_t *dst, uint64_t ld_dst, const uint64_t *src, uint64_t ld_src, uint64_t n, uint64_t ncols,
                     int inverse)
{
    int rc;
    if ((rc = require_init())) return rc;
    return ntt_dev(dst, ld_dst, src, ld_src, n, ncols, inverse);
}

uint64_t zkgpu_lde_workspace_bytes(uint64_t n, uint64_t n_ext, uint64_t ncols)
{
    return lde_workspace_bytes(n, n_ext, ncols);
}

void zkgpu_set_lde_batch_cols(uint64_t max_cols) { g_lde_batch_max = max_cols; }

int zkgpu_gl_extend_pol_dev(uint64_t *out, uint64_t ld_out, const uint64_t *in, uint64_t ld_in, uint64_t n_ext,
                            uint64_t n, uint64_t ncols)
{
    int rc;
    if ((rc = require_init())) return rc;
    return extend_pol_dev(out, ld_out, in, ld_in, n_ext, n, ncols);
}

int zkgpu_gl_extend_pol_inplace_dev(uint64_t *base, uint64_t n_ext, uint64_t n, uint64_t ncols)
{
    int rc;
    if ((rc = require_init())) return rc;
    if (!ncols || !n) return 0;
    if (!is_pow2(n) || !is_pow2(n_ext) || n_ext < n)
        return set_error(ZKGPU_ERR_ARG, "extend_pol_inplace: sizes must be powers of two with n_ext >= n");
    // batch [c0, c1) reads [c0 n, c1 n) and writes [c0 n_ext, c1 n_ext):
    // the columns below c0, still unread, end at c0 n <= c0 n_ext; within a
    // batch extend_pol_dev stages the whole input (coefficients in workspace
    // 0) before the first output store, on one stream
    const uint64_t batch = lde_batch_cols(n_ext, ncols);
    for (uint64_t c1 = ncols; c1 > 0;) {
        const uint64_t c0 = c1 > batch ? c1 - batch : 0;
        if ((rc = extend_pol_dev(base + c0 * n_ext, n_ext, base + c0 * n, n, n_ext, n, c1 - c0))) return rc;
        c1 = c0;
    }
    return 0;
}

int zkgpu_rows_to_cols_dev(uint64_t *cols, uint64_t ld, const uint64_t *rows, uint64_t nrows, uint64_t ncols)
{
    int rc;
    if ((rc = require_init())) return rc;
    rows_to_cols(rows, cols, nrows, ncols, ld, g_ctx.stream);
    return check_launch("rows_to_cols");
}

int zkgpu_cols_to_rows_dev(uint64_t *rows, const uint64_t *cols, uint64_t ld, uint64_t nrows, uint64_t ncols)
{
    int rc;
    if ((rc = require_init())) return rc;
    cols_to_rows(cols, rows, nrows, ncols, ld, g_ctx.stream);
    return check_launch("cols_to_rows");
}

// host-pointer drop-ins: H2D row-major -> column-major on device -> kernels
// -> row-major -> D2H.  Staging buffers: ws[2] (input cols), ws[3] (output).
int zkgpu_gl_ntt(uint64_t *dst, const uint64_t *src, uint64_t n, uint64_t ncols, int inverse)
{
    int rc;
    if ((rc = require_init())) return rc;
    if (!n || !ncols) return 0;
    Ctx &c = g_ctx;
    size_t bytes = n * ncols * sizeof(uint64_t);
    uint64_t *rows = workspace(2, bytes);
    uint64_t *cols = workspace(3, bytes);
    if (!rows || !cols) return ZKGPU_ERR_OOM;
    if ((rc = check_hip(hipMemcpyAsync(rows, src, bytes, hipMemcpyHostToDevice, c.stream), "H2D"))) return rc;
    rows_to_cols(rows, cols, n, ncols, n, c.stream);
    if ((rc = ntt_dev(cols, n, cols, n, n, ncols, inverse))) return rc;
    cols_to_rows(cols, rows, n, ncols, n, c.stream);
    if ((rc = check_hip(hipMemcpyAsync(dst, rows, bytes, hipMemcpyDeviceToHost, c.stream), "D2H"))) return rc;
    return check_hip(hipStreamSynchronize(c.stream), "ntt sync");
}

int zkgpu_gl_extend_pol(uint64_t *out, const uint64_t *in, uint64_t n_ext, uint64_t n, uint64_t ncols)
{
    int rc;
    if ((rc = require_init())) return rc;
    if (!n || !ncols) return 0;
    if (n_ext < n) return set_error(ZKGPU_ERR_ARG, "extend_pol: n_ext < n");
    Ctx &c = g_ctx;
    size_t in_bytes = n * ncols * sizeof(uint64_t), out_bytes = n_ext * ncols * sizeof(uint64_t);
    uint64_t *rows = workspace(2, out_bytes);
    uint64_t *cols = workspace(3, out_bytes + in_bytes);
    if (!rows || !cols) return ZKGPU_ERR_OOM;
    uint64_t *cin = cols + n_ext * ncols;
    if ((rc = check_hip(hipMemcpyAsync(rows, in, in_bytes, hipMemcpyHostToDevice, c.stream), "H2D"))) return rc;
    rows_to_cols(rows, cin, n, ncols, n, c.stream);
    if ((rc = extend_pol_dev(cols, n_ext, cin, n, n_ext, n, ncols))) return rc;
    cols_to_rows(cols, rows, n_ext, ncols, n_ext, c.stream);
    if ((rc = check_hip(hipMemcpyAsync(out, rows, out_bytes, hipMemcpyDeviceToHost, c.stream), "D2H"))) return rc;
    return check_hip(hipStreamSynchronize(c.stream), "extend_pol sync");
}

// ---------------------------------------------------------------- Poseidon
static int poseidon_one(uint64_t *out, const uint64_t *in, int full)
{
    int rc;
    if ((rc = require_init())) return rc;
    Ctx &c = g_ctx;
    uint64_t *d = workspace(2, 24 * sizeof(uint64_t));
    if (!d) return ZKGPU_ERR_OOM;
    if ((rc = check_hip(hipMemcpyAsync(d, in, 12 * sizeof(uint64_t), hipMemcpyHostToDevice, c.stream), "H2D")))
        return rc;
    if ((rc = poseidon_batch(d + 12, d, 1, full, c.stream))) return rc;
    if ((rc = check_hip(hipMemcpyAsync(out, d + 12, (full ? 12 : 4) * sizeof(uint64_t), hipMemcpyDeviceToHost,
                                       c.stream),
                        "D2H")))
        return rc;
    return check_hip(hipStreamSynchronize(c.stream), "poseidon sync");
}

int zkgpu_gl_poseidon_full(uint64_t out[12], const uint64_t in[12]) { return poseidon_one(out, in, 1); }

static uint64_t hp_pow7(uint64_t x)
{
    const uint64_t x2 = h_mul(x, x), x3 = h_mul(x2, x), x4 = h_mul(x2, x2);
    return h_mul(x3, x4);
}
// full round r: constants, x^7 on every lane, M[i][j] = MCIRC[(j - i) mod 12] +
// (i == j == 0) * 8 (an MDS row: 13 products of a canonical lane and a
// constant < 2^6, < 2^74, one fold of 2^64)
static void hp_full_round(uint64_t st[12], int r)
{
    static const uint32_t MC[12] = {17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20};
    for (int i = 0; i < 12; i++) st[i] = hp_pow7(h_add(st[i], ZKGPU_POSEIDON_RC[r * 12 + i]));
    uint64_t t[12];
    for (int i = 0; i < 12; i++) {
        unsigned __int128 acc = (i == 0) ? (unsigned __int128)st[0] * 8 : 0;
        for (int j = 0; j < 12; j++) acc += (unsigned __int128)st[j] * MC[j >= i ? j - i : j + 12 - i];
        const uint64_t lo = (uint64_t)acc, hi = (uint64_t)(acc >> 64);  // hi < 2^10
        const uint64_t hv = (hi << 32) - hi;                            // hi * 2^64 mod p
        uint64_t v = lo + hv;
        if (v < hv) v += 0xFFFFFFFFULL;
        t[i] = v >= HP ? v - HP : v;
    }
    memcpy(st, t, sizeof t);
}

// Host permutation for the transcript (PoseidonGoldilocks::hash_full_result
// on the CPU, transcript.cpp:18-24; the rounds of
// poseidon_g_executor.cpp:201-231): 4 full rounds, the 22 partial rounds in
// the sparse form the device uses (poseidon_gl_sparse.h, perm_sparse in
// csrc/poseidon_perm.hpp: 27 products per round instead of a 12x12 MDS),
// 4 full rounds.  Needs no GPU and no zkgpu_init.
int zkgpu_gl_poseidon_full_host(uint64_t out[12], const uint64_t in[12])
{
    uint64_t st[12];
    for (int i = 0; i < 12; i++) st[i] = in[i] % HP;
    for (int r = 0; r < 4; r++) hp_full_round(st, r);
    {
        uint64_t v[11];
        for (int j = 0; j < 11; j++) v[j] = h_add(st[1 + j], ZKGPU_PSP_PRE[1 + j]);
        st[0] = h_add(st[0], ZKGPU_PSP_PRE[0]);
        for (int i = 0; i < 11; i++) {
            uint64_t acc = 0;
            for (int j = 0; j < 11; j++) acc = h_add(acc, h_mul(v[j], ZKGPU_PSP_D0[i * 11 + j]));
            st[1 + i] = acc;
        }
    }
    for (int k = 0; k < 22; k++) {
        const uint64_t s0 = h_add(hp_pow7(st[0]), ZKGPU_PSP_POST[k]);
        uint64_t acc = h_mul(s0, 25);
        for (int j = 0; j < 11; j++) acc = h_add(acc, h_mul(st[1 + j], ZKGPU_PSP_W[k * 11 + j]));
        for (int j = 0; j < 11; j++) st[1 + j] = h_add(st[1 + j], h_mul(s0, ZKGPU_PSP_V[k * 11 + j]));
        st[0] = acc;
    }
    for (int r = 26; r < 30; r++) hp_full_round(st, r);
    memcpy(out, st, sizeof st);
    return 0;
}
int zkgpu_gl_poseidon_hash(uint64_t out[4], const uint64_t in[12]) { return poseidon_one(out, in, 0); }

int zkgpu_gl_poseidon_batch_dev(uint64_t *out, const uint64_t *in, uint64_t n, int full)
{
    int rc;
    if ((rc = require_init())) return rc;
    return poseidon_batch(out, in, n, full, g_ctx.stream);
}

int zkgpu_gl_linear_hash(uint64_t out[4], const uint64_t *in, uint64_t size)
{
    int rc;
    if ((rc = require_init())) return rc;
    Ctx &c = g_ctx;
    uint64_t *d = workspace(2, (size + 4) * sizeof(uint64_t));
    if (!d) return ZKGPU_ERR_OOM;
    if (size && (rc = check_hip(hipMemcpyAsync(d + 4, in, size * sizeof(uint64_t), hipMemcpyHostToDevice, c.stream),
                                "H2D")))
        return rc;
    // one row of `size` columns, column-major with ld = 1
    if ((rc = merkle_leaves_cols(d, d + 4, size, 1, 1, c.stream))) return rc;
    if ((rc = check_hip(hipMemcpyAsync(out, d, 4 * sizeof(uint64_t), hipMemcpyDeviceToHost, c.stream), "D2H")))
        return rc;
    return check_hip(hipStreamSynchronize(c.stream), "linear_hash sync");
}

// ---------------------------------------------------------------- Merkle
uint64_t zkgpu_gl_merkle_num_elements(uint64_t nrows) { return nrows ? 4 * nrows + 4 * (nrows - 1) : 0; }

int zkgpu_gl_merkletree_dev(uint64_t *nodes, const uint64_t *src, uint64_t ld, uint64_t ncols, uint64_t nrows)
{
    int rc;
    if ((rc = require_init())) return rc;
    if (!nrows) return 0;
    if (!is_pow2(nrows)) return set_error(ZKGPU_ERR_ARG, "merkletree: nrows must be a power of two");
    if ((rc = merkle_leaves_cols(nodes, src, ncols, nrows, ld, g_ctx.stream))) return rc;
    return merkle_levels(nodes, nrows, g_ctx.stream);
}

int zkgpu_gl_merkletree2_dev(uint64_t *nodes, const uint64_t *src, const uint64_t *src2, uint64_t ld, uint64_t split,
                             uint64_t ncols, uint64_t nrows)
{
    int rc;
    if ((rc = require_init())) return rc;
    if (!nrows) return 0;
    if (!is_pow2(nrows)) return set_error(ZKGPU_ERR_ARG, "merkletree2: nrows must be a power of two");
    if (split > ncols || (split < ncols && split % 8))
        return set_error(ZKGPU_ERR_ARG, "merkletree2: split %llu must be a multiple of 8 up to ncols",
                         (unsigned long long)split);
    if ((rc = merkle_leaves_cols(nodes, src, ncols, nrows, ld, g_ctx.stream, src2, split))) return rc;
    return merkle_levels(nodes, nrows, g_ctx.stream);
}

int zkgpu_gl_merkle_leaves_absorb_dev(uint64_t *nodes, const uint64_t *src, uint64_t ld, uint64_t col0, uint64_t ncols,
                                      uint64_t total_cols, uint64_t nrows)
{
    int rc;
    if ((rc = require_init())) return rc;
    if (col0 % 8)
        return set_error(ZKGPU_ERR_ARG, "merkle_leaves_absorb: col0 %llu must be a multiple of 8",
                         (unsigned long long)col0);
    if (col0 > total_cols || ncols > total_cols - col0)
        return set_error(ZKGPU_ERR_ARG, "merkle_leaves_absorb: columns [%llu, +%llu) outside the section's %llu",
                         (unsigned long long)col0, (unsigned long long)ncols, (unsigned long long)total_cols);
    if (total_cols <= 4 && ncols != total_cols)
        return set_error(ZKGPU_ERR_ARG, "merkle_leaves_absorb: a section of %llu <= 4 columns (copied, not hashed) "
                         "comes as one chunk", (unsigned long long)total_cols);
    if (col0 + ncols < total_cols && ncols % 8)
        return set_error(ZKGPU_ERR_ARG, "merkle_leaves_absorb: %llu columns: only the last chunk may not be a "
                         "multiple of 8", (unsigned long long)ncols);
    if (!ncols && total_cols) return set_error(ZKGPU_ERR_ARG, "merkle_leaves_absorb: an empty chunk");
    return merkle_leaves_absorb(nodes, src, ld, col0, ncols, total_cols, nrows, g_ctx.stream);
}

int zkgpu_gl_merkle_finish_dev(uint64_t *nodes, uint64_t nrows)
{
    int rc;
    if ((rc = require_init())) return rc;
    if (!nrows) return 0;
    if (!is_pow2(nrows)) return set_error(ZKGPU_ERR_ARG, "merkle_finish: nrows must be a power of two");
    return merkle_levels(nodes, nrows, g_ctx.stream);
}

int zkgpu_gl_merkletree_rows_dev(uint64_t *nodes, const uint64_t *src, uint64_t ncols, uint64_t nrows)
{
    int rc;
    if ((rc = require_init())) return rc;
    if (!nrows) return 0;
    if (!is_pow2(nrows)) return set_error(ZKGPU_ERR_ARG, "merkletree: nrows must be a power of two");
    if ((rc = merkle_leaves_rows(nodes, src, ncols, nrows, g_ctx.stream))) return rc;
    return merkle_levels(nodes, nrows, g_ctx.stream);
}

int zkgpu_gl_merkletree(uint64_t *nodes, const uint64_t *src, uint64_t ncols, uint64_t nrows)
{
    int rc;
    if ((rc = require_init())) return rc;
    if (!nrows) return 0;
    if (!is_pow2(nrows)) return set_error(ZKGPU_ERR_ARG, "merkletree: nrows must be a power of two");
    Ctx &c = g_ctx;
    size_t src_bytes = nrows * ncols * sizeof(uint64_t);
    size_t nodes_bytes = zkgpu_gl_merkle_num_elements(nrows) * sizeof(uint64_t);
    uint64_t *rows = workspace(2, src_bytes + 8);
    uint64_t *dn = workspace(3, nodes_bytes + src_bytes + 8);
    if (!rows || !dn) return ZKGPU_ERR_OOM;
    uint64_t *cols = dn + zkgpu_gl_merkle_num_elements(nrows);
    if (src_bytes &&
        (rc = check_hip(hipMemcpyAsync(rows, src, src_bytes, hipMemcpyHostToDevice, c.stream), "H2D")))
        return rc;
    rows_to_cols(rows, cols, nrows, ncols, nrows, c.stream);
    if ((rc = merkle_leaves_cols(dn, cols, ncols, nrows, nrows, c.stream))) return rc;
    if ((rc = merkle_levels(dn, nrows, c.stream))) return rc;
    if ((rc = check_hip(hipMemcpyAsync(nodes, dn, nodes_bytes, hipMemcpyDeviceToHost, c.stream), "D2H"))) return rc;
    return check_hip(hipStreamSynchronize(c.stream), "merkletree sync");
}

int zkgpu_gl_merkle_open_dev(uint64_t *vals_out, uint64_t *sibs_out, const uint64_t *nodes, const uint64_t *src,
                             uint64_t ld, uint64_t ncols, uint64_t nrows, const uint64_t *idx, uint64_t nq)
{
    int rc;
    if ((rc = require_init())) return rc;
    if (!nq) return 0;
    Ctx &c = g_ctx;
    if (nrows == 0 || (nrows & (nrows - 1)))
        return set_error(ZKGPU_ERR_ARG, "merkle_open: nrows %llu is not a power of two", (unsigned long long)nrows);
    uint32_t nlev = log2u(nrows);
    for (uint64_t q = 0; q < nq; q++)
        if (idx[q] >= nrows) return set_error(ZKGPU_ERR_ARG, "merkle_open: index %llu >= nrows", (unsigned long long)idx[q]);
    size_t nv = nq * ncols, ns = nq * nlev * 4;
    uint64_t *d = workspace(2, (nq + nv + ns + 1) * sizeof(uint64_t));
    if (!d) return ZKGPU_ERR_OOM;
    uint64_t *didx = d, *dv = d + nq, *ds = d + nq + nv;
    if ((rc = check_hip(hipMemcpyAsync(didx, idx, nq * sizeof(uint64_t), hipMemcpyHostToDevice, c.stream), "H2D")))
        return rc;
    if ((rc = merkle_open_cols(dv, ds, nodes, src, ncols, nrows, ld, didx, nq, c.stream))) return rc;
    if (nv && (rc = check_hip(hipMemcpyAsync(vals_out, dv, nv * sizeof(uint64_t), hipMemcpyDeviceToHost, c.stream),
                              "D2H")))
        return rc;
    if (ns && (rc = check_hip(hipMemcpyAsync(sibs_out, ds, ns * sizeof(uint64_t), hipMemcpyDeviceToHost, c.stream),
                              "D2H")))
        return rc;
    return check_hip(hipStreamSynchronize(c.stream), "merkle_open sync");
}

// ---------------------------------------------------------------- const tree
uint64_t zkgpu_const_tree_num_elements(uint64_t n_pols, uint32_t n_bits_ext)
{
    const uint64_t n_ext = 1ULL << n_bits_ext;
    return 2 + n_pols * n_ext + zkgpu_gl_merkle_num_elements(n_ext);
}

int zkgpu_build_const_tree(uint64_t *tree_out, const uint64_t *const_pols, uint64_t n_pols, uint32_t n_bits,
                           uint32_t n_bits_ext)
{
    int rc;
    if ((rc = require_init())) return rc;
    if (n_bits_ext < n_bits || n_bits_ext > TW_MAX_LOG)
        return set_error(ZKGPU_ERR_ARG, "const_tree: bad nBits %u / nBitsExt %u", n_bits, n_bits_ext);
    Ctx &c = g_ctx;
    const uint64_t n = 1ULL << n_bits, n_ext = 1ULL << n_bits_ext;
    const uint64_t n_nodes = zkgpu_gl_merkle_num_elements(n_ext);
    tree_out[0] = n_pols;  // Goldilocks::fromU64(nPols), fromU64(nExt)
    tree_out[1] = n_ext;
    const size_t in_bytes = n * n_pols * sizeof(uint64_t), out_bytes = n_ext * n_pols * sizeof(uint64_t);
    uint64_t *rows = workspace(2, out_bytes + 8);
    uint64_t *cols = workspace(3, out_bytes + in_bytes + n_nodes * sizeof(uint64_t) + 8);
    if (!rows || !cols) return ZKGPU_ERR_OOM;
    uint64_t *cin = cols + n_ext * n_pols;
    uint64_t *nodes = cin + n * n_pols;
    if (n_pols) {
        if ((rc = check_hip(hipMemcpyAsync(rows, const_pols, in_bytes, hipMemcpyHostToDevice, c.stream), "H2D")))
            return rc;
        rows_to_cols(rows, cin, n, n_pols, n, c.stream);
        if ((rc = extend_pol_dev(cols, n_ext, cin, n, n_ext, n, n_pols))) return rc;  // interpolate()
    }
    if ((rc = merkle_leaves_cols(nodes, cols, n_pols, n_ext, n_ext, c.stream))) return rc;
    if ((rc = merkle_levels(nodes, n_ext, c.stream))) return rc;
    if (n_pols) {
        cols_to_rows(cols, rows, n_ext, n_pols, n_ext, c.stream);
        if ((rc = check_hip(hipMemcpyAsync(tree_out + 2, rows, out_bytes, hipMemcpyDeviceToHost, c.stream), "D2H")))
            return rc;
    }
    if ((rc = check_hip(hipMemcpyAsync(tree_out + 2 + n_ext * n_pols, nodes, n_nodes * sizeof(uint64_t),
                                       hipMemcpyDeviceToHost, c.stream),
                        "D2H")))
        return rc;
    return check_hip(hipStreamSynchronize(c.stream), "const_tree sync");
}

// ---------------------------------------------------------------- executor hand-off
// block loop of the loaders: block b's H2D copy into stage half b & 1 on a copy
// stream, its transpose into the columns on stream ts once copied; a half is
// refilled only after its transpose has read it.  Returns with the work queued
// (ts, the copy stream), not finished.
// The load takes the window [col0, col0 + wcols) of the ncols-wide rows into
// columns cols + c*ld (c < wcols): a block's copy is then a strided one (host
// pitch ncols words, wcols words wide), packed in the stage; the whole width
// stays the one contiguous copy.  `nb` counts the blocks these streams and
// events have carried (several windows may share them: the streamed loader
// below), `half_words` is the fixed distance of the stage's halves.
struct LoadLane {
    hipStream_t cs = nullptr, ts = nullptr;
    hipEvent_t copied[2] = {nullptr, nullptr}, freed[2] = {nullptr, nullptr};
    uint64_t *stage = nullptr;
    uint64_t half_words = 0, nb = 0;
};

static int load_rows_blocks(LoadLane &L, uint64_t *cols, uint64_t ld, const uint64_t *rows, uint64_t nrows,
                            uint64_t ncols, uint64_t col0, uint64_t wcols, uint64_t block_rows)
{
    int rc = 0;
    const uint64_t nblocks = (nrows + block_rows - 1) / block_rows;
    for (uint64_t b = 0; b < nblocks && !rc; b++, L.nb++) {
        const int k = (int)(L.nb & 1);
        const uint64_t r0 = b * block_rows, nr = std::min(block_rows, nrows - r0);
        uint64_t *buf = L.stage + (size_t)k * L.half_words;
        const uint64_t *src = rows + r0 * ncols + col0;
        if (L.nb >= 2 && (rc = check_hip(hipStreamWaitEvent(L.cs, L.freed[k], 0), "wait"))) break;
        if (wcols == ncols)
            rc = check_hip(hipMemcpyAsync(buf, src, nr * ncols * sizeof(uint64_t), hipMemcpyHostToDevice, L.cs), "H2D");
        else
            rc = check_hip(hipMemcpy2DAsync(buf, wcols * sizeof(uint64_t), src, ncols * sizeof(uint64_t),
                                            wcols * sizeof(uint64_t), nr, hipMemcpyHostToDevice, L.cs),
                           "H2D (window)");
        if (rc) break;
        if ((rc = check_hip(hipEventRecord(L.copied[k], L.cs), "record"))) break;
        if ((rc = check_hip(hipStreamWaitEvent(L.ts, L.copied[k], 0), "wait"))) break;
        rows_to_cols(buf, cols + r0, nr, wcols, ld, L.ts);
        if ((rc = check_hip(hipEventRecord(L.freed[k], L.ts), "record"))) break;
    }
    return rc;
}

static uint64_t load_block_rows(uint64_t block_rows, uint64_t nrows, uint64_t ncols)
{
    if (!block_rows) block_rows = std::max<uint64_t>(1, (64ULL << 20) / (ncols * sizeof(uint64_t)));  // ~64 MB
    return std::min(block_rows, nrows);
}

// the copy stream and the events of a lane whose ts and stage are set
// `after` (optional): an event both streams wait for before their first
// command -- the background loader's streams are non-blocking and would
// otherwise overtake work the caller queued on the library stream into the
// same buffers (the zeroing memsets of freshly allocated cols / stage).
static int lane_open(LoadLane &L, hipEvent_t after)
{
    int rc = check_hip(hipStreamCreateWithFlags(&L.cs, hipStreamNonBlocking), "copy stream");
    for (int k = 0; k < 2 && !rc; k++) {
        rc = check_hip(hipEventCreateWithFlags(&L.copied[k], hipEventDisableTiming), "event");
        if (!rc) rc = check_hip(hipEventCreateWithFlags(&L.freed[k], hipEventDisableTiming), "event");
    }
    if (!rc && after) rc = check_hip(hipStreamWaitEvent(L.cs, after, 0), "wait");
    if (!rc && after) rc = check_hip(hipStreamWaitEvent(L.ts, after, 0), "wait");
    return rc;
}
// waits for the copy stream, then frees what lane_open made
static void lane_close(LoadLane &L)
{
    if (L.cs) (void)hipStreamSynchronize(L.cs);
    for (int k = 0; k < 2; k++) {
        if (L.copied[k]) (void)hipEventDestroy(L.copied[k]);
        if (L.freed[k]) (void)hipEventDestroy(L.freed[k]);
        L.copied[k] = L.freed[k] = nullptr;
    }
    if (L.cs) (void)hipStreamDestroy(L.cs);
    L.cs = nullptr;
}

// one load on its own streams (transposes on ts): the shared body of the
// synchronous and the background loader
static int load_rows_streams(uint64_t *cols, uint64_t ld, const uint64_t *rows, uint64_t nrows, uint64_t ncols,
                             uint64_t col0, uint64_t wcols, uint64_t block_rows, uint64_t *stage, hipStream_t ts,
                             bool register_host, hipEvent_t after = nullptr)
{
    int rc = 0;
    const size_t total = nrows * ncols * sizeof(uint64_t);
    bool registered = false;
    if (register_host) {
        if ((rc = check_hip(hipHostRegister((void *)rows, total, hipHostRegisterDefault), "hipHostRegister")))
            return rc;
        registered = true;
    }
    LoadLane L;
    L.ts = ts;
    L.stage = stage;
    L.half_words = block_rows * wcols;
    rc = lane_open(L, after);
    if (!rc) rc = load_rows_blocks(L, cols, ld, rows, nrows, ncols, col0, wcols, block_rows);
    if (!rc) rc = check_hip(hipStreamSynchronize(ts), "load_rows sync");
    lane_close(L);
    if (registered) (void)hipHostUnregister((void *)rows);
    return rc ? rc : check_launch("rows_to_cols");
}

int zkgpu_load_rows_dev(uint64_t *cols, uint64_t ld, const uint64_t *rows, uint64_t nrows, uint64_t ncols,
                        uint64_t block_rows, int register_host)
{
    return zkgpu_load_rows_window_dev(cols, ld, rows, nrows, ncols, 0, ncols, block_rows, register_host);
}

int zkgpu_load_rows_window_dev(uint64_t *cols, uint64_t ld, const uint64_t *rows, uint64_t nrows, uint64_t ncols,
                               uint64_t col0, uint64_t wcols, uint64_t block_rows, int register_host)
{
    int rc;
    if ((rc = require_init())) return rc;
    if (col0 > ncols || wcols > ncols - col0)
        return set_error(ZKGPU_ERR_ARG, "load_rows: window [%llu, +%llu) outside the %llu columns",
                         (unsigned long long)col0, (unsigned long long)wcols, (unsigned long long)ncols);
    if (!nrows || !wcols) return 0;
    if (ld < nrows) return set_error(ZKGPU_ERR_ARG, "load_rows: ld %llu < nrows", (unsigned long long)ld);
    block_rows = load_block_rows(block_rows, nrows, wcols);
    uint64_t *stage = workspace(2, 2 * block_rows * wcols * sizeof(uint64_t));
    if (!stage) return ZKGPU_ERR_OOM;
    return load_rows_streams(cols, ld, rows, nrows, ncols, col0, wcols, block_rows, stage, g_ctx.stream,
                             register_host != 0);
}

// Streamed loader (zkgpu_load_stream_*): windows of one host buffer queued one
// after another on a lane that lives across them, from the caller's thread.
struct LoadStream {
    LoadLane lane;
    const uint64_t *rows = nullptr;
    uint64_t nrows = 0, ncols = 0, windows = 0;
    long fail_at = -1;  // ZKGPU_STREAM_FAIL_BATCH (tests): window() fails before queuing this one
    hipEvent_t after = nullptr, done = nullptr;
    bool registered = false;
};

int zkgpu_load_stream_open(void **loader, const uint64_t *rows, uint64_t nrows, uint64_t ncols, uint64_t *stage,
                           uint64_t stage_bytes, int register_host)
{
    int rc;
    *loader = nullptr;
    if ((rc = require_init())) return rc;
    if (!rows || !nrows || !ncols || !stage || stage_bytes < 16)
        return set_error(ZKGPU_ERR_ARG, "load_stream_open: empty buffer or stage");
    LoadStream *s = new (std::nothrow) LoadStream();
    if (!s) return set_error(ZKGPU_ERR_OOM, "load_stream_open: loader");
    s->rows = rows;
    s->nrows = nrows;
    s->ncols = ncols;
    s->lane.stage = stage;
    s->lane.half_words = stage_bytes / 16;
    if (const char *e = getenv("ZKGPU_STREAM_FAIL_BATCH")) s->fail_at = strtol(e, nullptr, 10);
    if (register_host) {
        rc = check_hip(hipHostRegister((void *)rows, nrows * ncols * sizeof(uint64_t), hipHostRegisterDefault),
                       "hipHostRegister");
        s->registered = !rc;
    }
    if (!rc) rc = check_hip(hipStreamCreateWithFlags(&s->lane.ts, hipStreamNonBlocking), "loader stream");
    if (!rc) rc = check_hip(hipEventCreateWithFlags(&s->after, hipEventDisableTiming), "event");
    if (!rc) rc = check_hip(hipEventCreateWithFlags(&s->done, hipEventDisableTiming), "event");
    if (!rc) rc = check_hip(hipEventRecord(s->after, g_ctx.stream), "record");
    if (!rc) rc = lane_open(s->lane, s->after);
    if (rc) {
        char msg[sizeof g_err];
        snprintf(msg, sizeof msg, "%s", g_err);
        (void)zkgpu_load_stream_close(s);
        return set_error(rc, "%s", msg);
    }
    *loader = s;
    return 0;
}

int zkgpu_load_stream_window(void *loader, uint64_t *cols, uint64_t ld, uint64_t col0, uint64_t wcols)
{
    LoadStream *s = (LoadStream *)loader;
    if (!s) return set_error(ZKGPU_ERR_ARG, "load_stream_window: no loader");
    if (col0 > s->ncols || wcols > s->ncols - col0 || !wcols)
        return set_error(ZKGPU_ERR_ARG, "load_stream_window: window [%llu, +%llu) outside the %llu columns",
                         (unsigned long long)col0, (unsigned long long)wcols, (unsigned long long)s->ncols);
    if (ld < s->nrows) return set_error(ZKGPU_ERR_ARG, "load_stream_window: ld %llu < nrows", (unsigned long long)ld);
    if (s->lane.half_words < wcols)
        return set_error(ZKGPU_ERR_ARG, "load_stream_window: a stage half of %llu words holds no row of %llu columns",
                         (unsigned long long)s->lane.half_words, (unsigned long long)wcols);
    if ((long)s->windows == s->fail_at)
        return set_error(ZKGPU_ERR_HIP, "load_stream_window: injected failure before batch %ld (ZKGPU_STREAM_FAIL_BATCH)",
                         s->fail_at);
    s->windows++;
    const uint64_t block_rows = std::min(s->nrows, s->lane.half_words / wcols);
    int rc = load_rows_blocks(s->lane, cols, ld, s->rows, s->nrows, s->ncols, col0, wcols, block_rows);
    // recorded before the wait is queued, by this thread: the wait is for this window
    if (!rc) rc = check_hip(hipEventRecord(s->done, s->lane.ts), "record");
    if (!rc) rc = check_hip(hipStreamWaitEvent(g_ctx.stream, s->done, 0), "wait");
    return rc ? rc : check_launch("rows_to_cols");
}

int zkgpu_load_stream_close(void *loader)
{
    LoadStream *s = (LoadStream *)loader;
    if (!s) return 0;
    int rc = 0;
    if (s->lane.ts) rc = check_hip(hipStreamSynchronize(s->lane.ts), "load_stream sync");
    lane_close(s->lane);
    if (s->lane.ts) (void)hipStreamDestroy(s->lane.ts);
    if (s->after) (void)hipEventDestroy(s->after);
    if (s->done) (void)hipEventDestroy(s->done);
    if (s->registered) (void)hipHostUnregister((void *)s->rows);
    delete s;
    return rc;
}

// Background loader (zkgpu_load_rows_async): the same block loop in a host
// thread of its own, on streams of its own, so a proof's kernels on the
// library stream run while the next trace crosses PCIe.  A pageable source
// is staged through the driver by the calling thread of the copy, which is
// why the copies need a thread and not only a stream.
struct LoadTicket {
    std::thread th;
    int rc = 0;
    hipEvent_t after = nullptr;  // the library stream's work queued before the load
    char err[512] = "";          // the loader thread's error text (g_err is thread-local)
};

uint64_t zkgpu_load_rows_stage_bytes(uint64_t nrows, uint64_t ncols, uint64_t block_rows)
{
    if (!nrows || !ncols) return 0;
    return 2 * load_block_rows(block_rows, nrows, ncols) * ncols * sizeof(uint64_t);
}

int zkgpu_load_rows_async(uint64_t *cols, uint64_t ld, const uint64_t *rows, uint64_t nrows, uint64_t ncols,
                          uint64_t block_rows, uint64_t *stage, uint64_t stage_bytes, void **ticket)
{
    int rc;
    *ticket = nullptr;
    if ((rc = require_init())) return rc;
    if (ld < nrows) return set_error(ZKGPU_ERR_ARG, "load_rows_async: ld %llu < nrows", (unsigned long long)ld);
    block_rows = load_block_rows(block_rows, nrows, ncols);
    if (nrows && ncols && (!stage || stage_bytes < 2 * block_rows * ncols * sizeof(uint64_t)))
        return set_error(ZKGPU_ERR_ARG, "load_rows_async: stage of %llu bytes < 2 blocks (%llu)",
                         (unsigned long long)stage_bytes, (unsigned long long)(2 * block_rows * ncols * 8));
    LoadTicket *t = new (std::nothrow) LoadTicket();
    if (!t) return set_error(ZKGPU_ERR_OOM, "load_rows_async: ticket");
    if (nrows && ncols) {
        if ((rc = check_hip(hipEventCreateWithFlags(&t->after, hipEventDisableTiming), "event")) ||
            (rc = check_hip(hipEventRecord(t->after, g_ctx.stream), "record"))) {
            if (t->after) (void)hipEventDestroy(t->after);
            delete t;
            return rc;
        }
    }
    const int device = g_ctx.device;
    try {
        t->th = std::thread([=] {
        if (!nrows || !ncols) return;
        int r = check_hip(hipSetDevice(device), "hipSetDevice (loader)");
        hipStream_t ts = nullptr;
        if (!r) r = check_hip(hipStreamCreateWithFlags(&ts, hipStreamNonBlocking), "loader stream");
        if (!r) r = load_rows_streams(cols, ld, rows, nrows, ncols, 0, ncols, block_rows, stage, ts, false, t->after);
        if (ts) (void)hipStreamDestroy(ts);
        if (r) snprintf(t->err, sizeof t->err, "%s", g_err);
        t->rc = r;
        });
    } catch (...) {  // no thread: nothing started
        if (t->after) (void)hipEventDestroy(t->after);
        delete t;
        return set_error(ZKGPU_ERR_ARG, "load_rows_async: cannot start the loader thread");
    }
    *ticket = t;
    return 0;
}

int zkgpu_load_wait(void *ticket)
{
    if (!ticket) return 0;
    LoadTicket *t = (LoadTicket *)ticket;
    if (t->th.joinable()) t->th.join();
    const int rc = t->rc;
    if (rc) set_error(rc, "%s", t->err);  // the loader's message, on the waiting thread
    if (t->after) (void)hipEventDestroy(t->after);
    delete t;
    return rc;
}

// ---------------------------------------------------------------- device memory
int zkgpu_dev_malloc(void **ptr, uint64_t bytes)
{
    int rc;
    if ((rc = require_init())) return rc;
    if (hipMalloc(ptr, bytes ? bytes : 8) != hipSuccess) {
        *ptr = nullptr;
        return set_error(ZKGPU_ERR_OOM, "hipMalloc(%llu) failed", (unsigned long long)bytes);
    }
    return 0;
}
int zkgpu_dev_free(void *ptr) { return ptr ? check_hip(hipFree(ptr), "hipFree") : 0; }
int zkgpu_memcpy_h2d(void *dst, const void *src, uint64_t bytes)
{
    if (!bytes) return 0;
    int rc = check_hip(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, g_ctx.stream), "H2D");
    return rc ? rc : check_hip(hipStreamSynchronize(g_ctx.stream), "H2D sync");
}
int zkgpu_memcpy_d2h(void *dst, const void *src, uint64_t bytes)
{
    if (!bytes) return 0;
    int rc = check_hip(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, g_ctx.stream), "D2H");
    return rc ? rc : check_hip(hipStreamSynchronize(g_ctx.stream), "D2H sync");
}
int zkgpu_memcpy_d2d(void *dst, const void *src, uint64_t bytes)
{
    if (!bytes) return 0;
    return check_hip(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, g_ctx.stream), "D2D");
}
int zkgpu_memset_dev(void *dst, int value, uint64_t bytes)
{
    if (!bytes) return 0;
    return check_hip(hipMemsetAsync(dst, value, bytes, g_ctx.stream), "memset");
}

// ---------------------------------------------------------------- STARK stages
// small host arrays staged through a grow-only device buffer (ws slot 3 is the
// host-API staging area; stage params use their own allocation)
static uint64_t *g_param = nullptr;
static size_t g_param_bytes = 0;
static char *param_buf(size_t bytes)
{
    if (bytes > g_param_bytes) {
        (void)hipStreamSynchronize(g_ctx.stream);
        if (g_param) (void)hipFree(g_param);
        g_param = nullptr;
        if (hipMalloc((void **)&g_param, bytes) != hipSuccess) {
            g_param_bytes = 0;
            return nullptr;
        }
        g_param_bytes = bytes;
    }
    return (char *)g_param;
}

int zkgpu_rand_cols_dev(uint64_t *base, uint64_t ld, const uint32_t *cols, uint32_t ncols, uint64_t nrows,
                        uint64_t seed, uint64_t stream)
{
    int rc;
    if ((rc = require_init())) return rc;
    if (!ncols || !nrows) return 0;
    if (ncols > 65535 || nrows > ld) return set_error(ZKGPU_ERR_ARG, "rand_cols: bad shape");
    char *p = param_buf(ncols * 4);
    if (!p) return set_error(ZKGPU_ERR_OOM, "param buffer");
    if ((rc = check_hip(hipMemcpyAsync(p, cols, ncols * 4, hipMemcpyHostToDevice, g_ctx.stream), "H2D"))) return rc;
    if ((rc = check_hip(hipStreamSynchronize(g_ctx.stream), "rand_cols param upload"))) return rc;
    return rand_cols(base, ld, (const uint32_t *)p, ncols, nrows, seed, stream, 0, ~0ULL, g_ctx.stream);
}

int zkgpu_rand_cols_rows_dev(uint64_t *base, uint64_t ld, const uint32_t *cols, uint32_t ncols, uint64_t row0,
                             uint64_t nrows, uint32_t log_n, uint64_t seed, uint64_t stream)
{
    int rc;
    if ((rc = require_init())) return rc;
    if (!ncols || !nrows) return 0;
    if (log_n > 40 || ncols > 65535 || nrows > ld) return set_error(ZKGPU_ERR_ARG, "rand_cols_rows: bad shape");
    char *p = param_buf(ncols * 4);
    if (!p) return set_error(ZKGPU_ERR_OOM, "param buffer");
    if ((rc = check_hip(hipMemcpyAsync(p, cols, ncols * 4, hipMemcpyHostToDevice, g_ctx.stream), "H2D"))) return rc;
    if ((rc = check_hip(hipStreamSynchronize(g_ctx.stream), "rand_cols param upload"))) return rc;
    return rand_cols(base, ld, (const uint32_t *)p, ncols, nrows, seed, stream, row0, (1ULL << log_n) - 1,
                     g_ctx.stream);
}

int zkgpu_copy_rows_dev(uint64_t *dst, uint64_t dst_ld, uint64_t dst_row0, const uint32_t *dst_cols,
                        const uint64_t *src, uint64_t src_ld, uint64_t src_row0, uint32_t src_log_mod,
                        const uint32_t *src_cols, uint32_t ncols, uint64_t nrows)
{
    int rc;
    if ((rc = require_init())) return rc;
    if (!ncols || !nrows) return 0;
    if (!dst || !src || ncols > 65535 || src_log_mod > 63 || dst_row0 + nrows > dst_ld ||
        (!src_log_mod && src_row0 + nrows > src_ld) || (src_log_mod && (1ULL << src_log_mod) > src_ld))
        return set_error(ZKGPU_ERR_ARG, "copy_rows: rows outside the buffers' leading dimensions");
    const size_t nd = dst_cols ? ncols : 0, ns = src_cols ? ncols : 0;
    char *p = param_buf((nd + ns) * 4 + 8);
    if (!p) return set_error(ZKGPU_ERR_OOM, "param buffer");
    if (nd && (rc = check_hip(hipMemcpyAsync(p, dst_cols, nd * 4, hipMemcpyHostToDevice, g_ctx.stream), "H2D")))
        return rc;
    if (ns && (rc = check_hip(hipMemcpyAsync(p + nd * 4, src_cols, ns * 4, hipMemcpyHostToDevice, g_ctx.stream), "H2D")))
        return rc;
    if ((nd || ns) && (rc = check_hip(hipStreamSynchronize(g_ctx.stream), "copy_rows param upload"))) return rc;
    return copy_rows(dst, dst_ld, dst_row0, nd ? (const uint32_t *)p : nullptr, src, src_ld, src_row0,
                     src_log_mod ? (1ULL << src_log_mod) - 1 : ~0ULL, ns ? (const uint32_t *)(p + nd * 4) : nullptr,
                     ncols, nrows, g_ctx.stream);
}

int zkgpu_device_memory(uint64_t *free_bytes, uint64_t *total_bytes)
{
    int rc;
    if ((rc = require_init())) return rc;
    size_t f = 0, t = 0;
    if ((rc = check_hip(hipMemGetInfo(&f, &t), "hipMemGetInfo"))) return rc;
    if (free_bytes) *free_bytes = f;
    if (total_bytes) *total_bytes = t;
    return 0;
}

// zhInv tables (<= 64 words) on the device, one per (log omega, extend
// bits), uploaded once: the compiled expression kernels read them and need
// no per-call upload (and no stream sync for a pageable source)
// (keyed by device too: zkgpu_init may switch devices)
static const uint64_t *zh_table(uint32_t log_omega, uint32_t eb, const uint64_t *zhv, size_t n)
{
    static std::mutex mu;
    static std::map<std::pair<int, std::pair<uint32_t, uint32_t>>, uint64_t *> tabs;
    std::lock_guard<std::mutex> lk(mu);
    const auto key = std::make_pair(g_ctx.device, std::make_pair(log_omega, eb));
    auto it = tabs.find(key);
    if (it != tabs.end()) return it->second;
    uint64_t *d = nullptr;
    if (check_hip(hipMalloc((void **)&d, 64 * 8), "zxp: zhInv table")) return nullptr;
    if (check_hip(hipMemcpy(d, zhv, n * 8, hipMemcpyHostToDevice), "zxp: zhInv table")) {
        (void)hipFree(d);
        return nullptr;
    }
    tabs[key] = d;
    return d;
}

// One expression-program evaluation.  The host work -- argument checks, the
// plan, the interpreter's records -- is csrc/zxp_prepare.cpp; here are the
// device tables, the uploads and the launches.
static int zxp_eval_run(const ZxpArgs &a)
{
    int rc;
    if ((rc = require_init()) || (rc = zxp_validate(a))) return rc;
    ZxpPlan P;
    if ((rc = zxp_plan(a, P))) return rc;
    hipStream_t s = g_ctx.stream;
    const uint64_t x_start = a.x_start % HP;
    if (P.jit) {
        // the compiled kernels take their own tables (csrc/zxp_jit.hip): no
        // interpreter records, no upload or stream sync here, so the host
        // prepares them while earlier work still runs on the stream
        ZxpJitIn J = zxp_jit_in(P.prog, a.sections, a.challenges, a.publics, a.evals);
        // (the cached table is the real one: only a program that reads it asks for it)
        J.zh_dev = nullptr;
        if (P.uses_zi && !(J.zh_dev = zh_table(a.log_omega, a.extend_bits, P.zhinv, P.n_zhinv))) return -1;
        J.log_dom = a.log_dom;
        J.log_omega = a.log_omega;
        J.wrap = a.wrap ? 1u : 0u;
        J.xdiv = a.xdiv;
        J.xdivw = a.xdivw;
        J.zmask = P.n_zhinv - 1;
        J.x_start = x_start;
        J.bytes = P.bytes;
        if ((rc = zxp_jit_run(J, s)) <= 0) return rc;  // launched, or an error
        // 1 = shape unsupported: the interpreter runs the same plan
    }
    const size_t off_terms = (size_t)std::max<uint32_t>(P.prog.n_instr, 1) * sizeof(ZOp);
    const size_t off_zh = off_terms + (size_t)P.n_dot_terms * sizeof(ZTerm);
    char *p = param_buf(off_zh + P.n_zhinv * 8 + 16);
    if (!p) return set_error(ZKGPU_ERR_OOM, "param buffer");
    std::vector<ZOp> ops;
    std::vector<ZTerm> terms;
    if ((rc = zxp_records(a, P, (const uint64_t *)(p + off_zh), ops, terms))) return rc;
    if ((rc = check_hip(hipMemcpyAsync(p, ops.data(), ops.size() * sizeof(ZOp), hipMemcpyHostToDevice, s), "H2D")) ||
        (terms.size() && (rc = check_hip(hipMemcpyAsync(p + off_terms, terms.data(), terms.size() * sizeof(ZTerm),
                                                        hipMemcpyHostToDevice, s),
                                         "H2D"))) ||
        (rc = check_hip(hipMemcpyAsync(p + off_zh, P.zhinv, P.n_zhinv * 8, hipMemcpyHostToDevice, s), "H2D")))
        return rc;
    // the sources are pageable host memory (the plan lives on this stack): the
    // uploads must complete before returning
    if ((rc = check_hip(hipStreamSynchronize(s), "zxp param upload"))) return rc;
    ZxpLaunch L;
    L.prog = (const ZOp *)p;
    L.terms = (const ZTerm *)(p + off_terms);
    L.n_instr = P.prog.n_instr;
    L.n_tmp1 = P.prog.n_tmp1;
    L.n_tmp3 = P.prog.n_tmp3;
    L.logdom = a.log_dom;
    L.logomega = a.log_omega;
    L.wrap = a.wrap ? 1u : 0u;
    L.x_start = x_start;
    L.bytes = P.bytes;
    return zxp_eval(L, s);
}

int zkgpu_zxp_eval_dev(const void *instr, uint32_t n_instr, const void *opnd, uint32_t n_opnd, uint32_t n_tmp1,
                       uint32_t n_tmp3, const zkgpu_sections *sections, uint32_t log_dom, const uint64_t *challenges,
                       const uint64_t *publics, uint32_t n_publics, const uint64_t *evals, uint32_t n_evals,
                       const uint64_t *xdiv, const uint64_t *xdivw, uint32_t extend_bits, uint64_t x_start)
{
    return zxp_eval_run(ZxpArgs{(const zxp_instr *)instr, n_instr, (const zxp_operand *)opnd, n_opnd, n_tmp1, n_tmp3,
                                sections, log_dom, log_dom, 1, challenges, publics, n_publics, evals, n_evals, xdiv,
                                xdivw, extend_bits, x_start});
}

// zkgpu_zxp_eval_rows_dev runs inside a proof that must not wait for the host,
// so its records go up from PINNED staging buffers: a pair (host, device) of
// the current device is taken -- marked busy under the lock -- when it is
// large enough, not in a caller's hands, and the event recorded behind its
// last launch has completed; another pair is made when there is none (a
// hipMalloc waits for nothing).  The pairs sit in a deque, so a pair's address
// holds while others are added.  They live as long as the process, like
// g_param and the zhInv tables: at most one per call in flight, each of the
// size of one program's records.
struct RowsStage {
    int device;
    char *host, *dev;
    size_t bytes;
    hipEvent_t done;
    bool busy;  // between rows_stage and rows_stage_done
};
static std::deque<RowsStage> g_rows_stages;
static std::mutex g_rows_stages_mu;
static RowsStage *rows_stage(size_t bytes)
{
    std::lock_guard<std::mutex> lk(g_rows_stages_mu);
    for (RowsStage &r : g_rows_stages)
        if (r.device == g_ctx.device && !r.busy && r.bytes >= bytes && hipEventQuery(r.done) == hipSuccess) {
            r.busy = true;
            return &r;
        }
    RowsStage r{g_ctx.device, nullptr, nullptr, std::max<size_t>(bytes, 1 << 16), nullptr, true};
    if (hipHostMalloc((void **)&r.host, r.bytes, hipHostMallocDefault) != hipSuccess ||
        hipMalloc((void **)&r.dev, r.bytes) != hipSuccess ||
        hipEventCreateWithFlags(&r.done, hipEventDisableTiming) != hipSuccess) {
        if (r.host) (void)hipHostFree(r.host);
        if (r.dev) (void)hipFree(r.dev);
        return nullptr;
    }
    g_rows_stages.push_back(r);
    return &g_rows_stages.back();
}
// the caller is through with the pair: what it queued on s (if anything) ends at the event
static int rows_stage_done(RowsStage *st, hipStream_t s, bool queued)
{
    const int rc = queued ? check_hip(hipEventRecord(st->done, s), "zxp rows: event") : 0;
    std::lock_guard<std::mutex> lk(g_rows_stages_mu);
    st->busy = false;
    return rc;
}

// One evaluation at a list of rows: the phases of zxp_eval_run, always the
// interpreter, no host synchronisation.
static int zxp_eval_rows_run(const ZxpArgs &a)
{
    int rc;
    if ((rc = require_init()) || (rc = zxp_validate(a))) return rc;
    if (!a.n_rows) return 0;
    ZxpPlan P;
    if ((rc = zxp_plan(a, P))) return rc;
    hipStream_t s = g_ctx.stream;
    const size_t off_terms = (size_t)std::max<uint32_t>(P.prog.n_instr, 1) * sizeof(ZOp);
    const size_t off_zh = off_terms + (size_t)P.n_dot_terms * sizeof(ZTerm);
    const size_t bytes = off_zh + P.n_zhinv * 8;
    RowsStage *st = rows_stage(bytes);
    if (!st) return set_error(ZKGPU_ERR_OOM, "zxp rows: staging buffers");
    std::vector<ZOp> ops;
    std::vector<ZTerm> terms;
    if ((rc = zxp_records(a, P, (const uint64_t *)(st->dev + off_zh), ops, terms))) {
        (void)rows_stage_done(st, s, false);
        return rc;
    }
    if (ops.size()) memcpy(st->host, ops.data(), ops.size() * sizeof(ZOp));
    if (terms.size()) memcpy(st->host + off_terms, terms.data(), terms.size() * sizeof(ZTerm));
    memcpy(st->host + off_zh, P.zhinv, P.n_zhinv * 8);
    if ((rc = check_hip(hipMemcpyAsync(st->dev, st->host, bytes, hipMemcpyHostToDevice, s), "H2D"))) {
        (void)rows_stage_done(st, s, true);
        return rc;
    }
    ZxpLaunch L;
    L.prog = (const ZOp *)st->dev;
    L.terms = (const ZTerm *)(st->dev + off_terms);
    L.n_instr = P.prog.n_instr;
    L.n_tmp1 = P.prog.n_tmp1;
    L.n_tmp3 = P.prog.n_tmp3;
    L.logdom = a.log_dom;
    L.logomega = a.log_omega;
    L.wrap = 1;
    L.x_start = a.x_start % HP;
    L.bytes = P.bytes;
    rc = zxp_eval_rows(L, a.rows, a.n_rows, s);
    // (recorded after a failed launch too: the copy still reads the host buffer)
    const int rc2 = rows_stage_done(st, s, true);
    return rc ? rc : rc2;
}

int zkgpu_zxp_eval_rows_dev(const void *instr, uint32_t n_instr, const void *opnd, uint32_t n_opnd, uint32_t n_tmp1,
                            uint32_t n_tmp3, const zkgpu_sections *sections, uint32_t log_dom,
                            const uint64_t *challenges, const uint64_t *publics, uint32_t n_publics,
                            const uint64_t *evals, uint32_t n_evals, const uint64_t *xdiv, const uint64_t *xdivw,
                            uint32_t extend_bits, uint64_t x_start, const uint64_t *rows, uint32_t n_rows)
{
    ZxpArgs a{(const zxp_instr *)instr, n_instr, (const zxp_operand *)opnd, n_opnd, n_tmp1, n_tmp3,
              sections, log_dom, log_dom, 1, challenges, publics, n_publics, evals, n_evals, xdiv,
              xdivw, extend_bits, x_start};
    a.row_list = true;
    a.rows = rows;
    a.n_rows = n_rows;
    return zxp_eval_rows_run(a);
}

int zkgpu_zxp_eval_block_dev(const void *instr, uint32_t n_instr, const void *opnd, uint32_t n_opnd, uint32_t n_tmp1,
                             uint32_t n_tmp3, const zkgpu_sections *sections, uint32_t log_rows, uint32_t log_domain,
                             const uint64_t *challenges, const uint64_t *publics, uint32_t n_publics,
                             const uint64_t *evals, uint32_t n_evals, const uint64_t *xdiv, const uint64_t *xdivw,
                             uint32_t extend_bits, uint64_t x_start)
{
    return zxp_eval_run(ZxpArgs{(const zxp_instr *)instr, n_instr, (const zxp_operand *)opnd, n_opnd, n_tmp1, n_tmp3,
                                sections, log_rows, log_domain, 0, challenges, publics, n_publics, evals, n_evals, xdiv,
                                xdivw, extend_bits, x_start});
}

int zkgpu_calculate_z_block_dev(uint64_t *z, uint64_t z_ld, const uint64_t *num, uint64_t num_ld, const uint64_t *den,
                                uint64_t den_ld, uint64_t n, const uint64_t z0[3], uint64_t total[3])
{
    int rc;
    if ((rc = require_init())) return rc;
    if (!z0 || !total) return set_error(ZKGPU_ERR_ARG, "calculate_z_block: null z0 / total");
    if (!n) {
        for (int k = 0; k < 3; k++) total[k] = z0[k] % HP;
        return 0;
    }
    if (z_ld < n || num_ld < n || den_ld < n) return set_error(ZKGPU_ERR_ARG, "calculate_z: ld < n");
    const size_t words = calculate_z_scratch_words(n);
    uint64_t *scr = workspace(2, (words + 8) * sizeof(uint64_t));
    if (!scr) return ZKGPU_ERR_OOM;
    uint64_t *tot = scr + words;
    if ((rc = calculate_z(z, z_ld, num, num_ld, den, den_ld, n, z0, scr, tot, g_ctx.stream))) return rc;
    if ((rc = check_hip(hipMemcpyAsync(total, tot, 24, hipMemcpyDeviceToHost, g_ctx.stream), "D2H"))) return rc;
    return check_hip(hipStreamSynchronize(g_ctx.stream), "calculateZ sync");
}

int zkgpu_calculate_z_many_dev(const zkgpu_z_req *req, uint32_t nz, uint64_t n, int *closes)
{
    int rc;
    if ((rc = require_init())) return rc;
    if (!nz) return 0;
    if (!req || !closes) return set_error(ZKGPU_ERR_ARG, "calculate_z_many: null argument");
    if (!n) {
        for (uint32_t k = 0; k < nz; k++) closes[k] = 1;  // an empty product
        return 0;
    }
    for (uint32_t k = 0; k < nz; k++)
        if (req[k].z_ld < n || req[k].num_ld < n || req[k].den_ld < n)
            return set_error(ZKGPU_ERR_ARG, "calculate_z_many: request %u: ld < n", k);
    // the requests run in stream order on one scratch; each keeps its total
    const size_t words = calculate_z_scratch_words(n);
    uint64_t *scr = workspace(2, (words + 3ULL * nz + 8) * sizeof(uint64_t));
    if (!scr) return ZKGPU_ERR_OOM;
    uint64_t *tot = scr + words;
    const uint64_t one[3] = {1, 0, 0};
    for (uint32_t k = 0; k < nz; k++)
        if ((rc = calculate_z(req[k].z, req[k].z_ld, req[k].num, req[k].num_ld, req[k].den, req[k].den_ld, n, one, scr,
                              tot + 3ULL * k, g_ctx.stream)))
            return rc;
    std::vector<uint64_t> t(3ULL * nz);
    if ((rc = check_hip(hipMemcpyAsync(t.data(), tot, t.size() * 8, hipMemcpyDeviceToHost, g_ctx.stream), "D2H")))
        return rc;
    if ((rc = check_hip(hipStreamSynchronize(g_ctx.stream), "calculateZ sync"))) return rc;
    for (uint32_t k = 0; k < nz; k++) closes[k] = (t[3 * k] == 1 && t[3 * k + 1] == 0 && t[3 * k + 2] == 0) ? 1 : 0;
    return 0;
}

int zkgpu_calculate_z_dev(uint64_t *z, uint64_t z_ld, const uint64_t *num, uint64_t num_ld, const uint64_t *den,
                          uint64_t den_ld, uint64_t n, int *closes)
{
    const uint64_t one[3] = {1, 0, 0};
    uint64_t tot[3] = {1, 0, 0};
    const int rc = zkgpu_calculate_z_block_dev(z, z_ld, num, num_ld, den, den_ld, n, one, tot);
    if (rc) return rc;
    // z[n-1] * num[n-1] / den[n-1] == 1: the product of every ratio
    if (closes) *closes = (tot[0] == 1 && tot[1] == 0 && tot[2] == 0) ? 1 : 0;
    return 0;
}

int zkgpu_evmap_dev(uint64_t *evals_out, const uint64_t *const *cols, const uint64_t *lds, const uint32_t *dims,
                    const uint32_t *primes, uint32_t n_ev, const uint64_t *lev, const uint64_t *lpev, uint64_t l_ld,
                    uint64_t n, uint32_t extend_bits)
{
    int rc;
    if ((rc = require_init())) return rc;
    if (!n_ev) return 0;
    for (uint32_t e = 0; e < n_ev; e++)
        if (dims[e] != 1 && dims[e] != 3) return set_error(ZKGPU_ERR_ARG, "evmap: entry %u dim %u", e, dims[e]);
    if (!n) {  // an empty row block: every sum is zero, nothing to launch
        memset(evals_out, 0, (size_t)n_ev * 24);
        return 0;
    }
    if (l_ld < n) return set_error(ZKGPU_ERR_ARG, "evmap: l_ld < n");
    if (extend_bits > 63 || ((n - 1) << extend_bits) >> extend_bits != n - 1)
        return set_error(ZKGPU_ERR_ARG, "evmap: rows << extend_bits beyond 2^64");
    // a dim-3 entry's components lie lds[e] apart: each must hold the last row read
    const uint64_t span = ((n - 1) << extend_bits) + 1;
    for (uint32_t e = 0; e < n_ev; e++)
        if (dims[e] == 3 && lds[e] < span)
            return set_error(ZKGPU_ERR_ARG, "evmap: entry %u: ld %llu < %llu rows", e, (unsigned long long)lds[e],
                             (unsigned long long)span);
    // sub-entries: a dim-1 entry is one, a dim-3 entry three (component j,
    // weighted by X^j when the sums are combined); grouped by L (prime or not)
    // into EV_G-wide groups
    struct G {
        const uint64_t *col[8];
        uint32_t prime, sub0;
    };
    if (evmap_group_size() != sizeof(G) || evmap_group_width() != 8) return set_error(ZKGPU_ERR_ARG, "evmap group layout");
    constexpr uint32_t GW = 4;  // sub-entries per group: accumulator VGPRs vs shared limb work
    constexpr uint32_t UR = 2;  // rows per thread and iteration
    struct Sub {
        const uint64_t *col;
        uint32_t prime, which, entry;
    };
    std::vector<Sub> subs;
    for (uint32_t e = 0; e < n_ev; e++)
        for (uint32_t j = 0; j < dims[e]; j++) subs.push_back(Sub{cols[e] + (uint64_t)j * lds[e], primes[e] ? 1u : 0u, j, e});
    std::stable_sort(subs.begin(), subs.end(), [](const Sub &a, const Sub &b) { return a.prime < b.prime; });
    std::vector<G> groups;
    std::vector<int32_t> sub_of(3 * (size_t)n_ev, -1);
    for (size_t i = 0; i < subs.size();) {
        G g;
        memset(&g, 0, sizeof(g));
        g.prime = subs[i].prime;
        g.sub0 = (uint32_t)i;
        uint32_t c = 0;
        while (c < GW && i < subs.size() && subs[i].prime == g.prime) {
            g.col[c++] = subs[i].col;
            sub_of[3 * (size_t)subs[i].entry + subs[i].which] = (int32_t)i;
            i++;
        }
        groups.push_back(g);
    }
    const uint64_t rpb = evmap_rows_per_block();
    const uint64_t nblk_ = (n + rpb - 1) / rpb;
    const size_t off_sub = (groups.size() * sizeof(G) + 15) & ~15ULL;
    const size_t off_part = (off_sub + sub_of.size() * 4 + 15) & ~15ULL;
    const size_t off_ev = off_part + subs.size() * nblk_ * 24;
    char *p = param_buf(off_ev + n_ev * 24);
    if (!p) return set_error(ZKGPU_ERR_OOM, "param buffer");
    if ((rc = check_hip(hipMemcpyAsync(p, groups.data(), groups.size() * sizeof(G), hipMemcpyHostToDevice,
                                       g_ctx.stream), "H2D")) ||
        (rc = check_hip(hipMemcpyAsync(p + off_sub, sub_of.data(), sub_of.size() * 4, hipMemcpyHostToDevice,
                                       g_ctx.stream), "H2D")) ||
        (rc = check_hip(hipStreamSynchronize(g_ctx.stream), "evmap param upload")))
        return rc;
    if ((rc = evmap_groups((uint64_t *)(p + off_ev), p, (uint32_t)groups.size(), GW, UR, (const int32_t *)(p + off_sub), n_ev,
                           (uint32_t)subs.size(), lev, lpev, l_ld, n, extend_bits, (uint64_t *)(p + off_part),
                           g_ctx.stream)))
        return rc;
    if ((rc = check_hip(hipMemcpyAsync(evals_out, p + off_ev, n_ev * 24, hipMemcpyDeviceToHost, g_ctx.stream), "D2H")))
        return rc;
    return check_hip(hipStreamSynchronize(g_ctx.stream), "evmap sync");
}

int zkgpu_xdivxsub_dev(uint64_t *xdiv, uint64_t *xdivw, const uint64_t xi[3], uint32_t n_bits, uint32_t n_bits_ext)
{
    int rc;
    if ((rc = require_init())) return rc;
    if (n_bits_ext > TW_MAX_LOG || n_bits > n_bits_ext) return set_error(ZKGPU_ERR_ARG, "xdivxsub: bits");
    return xdivxsub(xdiv, xdivw, xi, h_w(n_bits), n_bits_ext, g_ctx.stream);
}

int zkgpu_xdivxsub_rows_dev(uint64_t *xdiv, uint64_t *xdivw, const uint64_t xi[3], uint32_t n_bits,
                            uint32_t n_bits_ext, uint64_t row0, uint64_t nrows)
{
    int rc;
    if ((rc = require_init())) return rc;
    if (n_bits_ext > TW_MAX_LOG || n_bits > n_bits_ext) return set_error(ZKGPU_ERR_ARG, "xdivxsub_rows: bits");
    if (row0 > (1ULL << n_bits_ext) || nrows > (1ULL << n_bits_ext) - row0)
        return set_error(ZKGPU_ERR_ARG, "xdivxsub_rows: rows [%llu, +%llu) outside the domain",
                         (unsigned long long)row0, (unsigned long long)nrows);
    return xdivxsub_rows(xdiv, xdivw, xi, h_w(n_bits), n_bits_ext, row0, nrows, g_ctx.stream);
}

// F_p^3 helpers for the closed-form weights (host)
static void h3_mul(uint64_t r[3], const uint64_t a[3], const uint64_t b[3])
{
    // x^3 = x + 1
    const uint64_t c0 = h_mul(a[0], b[0]);
    const uint64_t c1 = (uint64_t)(((unsigned __int128)h_mul(a[0], b[1]) + h_mul(a[1], b[0])) % ZK_P);
    const uint64_t c2 =
        (uint64_t)(((unsigned __int128)h_mul(a[0], b[2]) + h_mul(a[1], b[1]) + h_mul(a[2], b[0])) % ZK_P);
    const uint64_t c3 = (uint64_t)(((unsigned __int128)h_mul(a[1], b[2]) + h_mul(a[2], b[1])) % ZK_P);
    const uint64_t c4 = h_mul(a[2], b[2]);
    r[0] = (uint64_t)(((unsigned __int128)c0 + c3) % ZK_P);
    r[1] = (uint64_t)(((unsigned __int128)c1 + c3 + c4) % ZK_P);
    r[2] = (uint64_t)(((unsigned __int128)c2 + c4) % ZK_P);
}

int zkgpu_lagrange_xi_rows_dev(uint64_t *lev, uint64_t *lpev, uint64_t ld, const uint64_t xi[3], uint32_t n_bits,
                               uint64_t row0, uint64_t nrows)
{
    int rc;
    if ((rc = require_init())) return rc;
    if (n_bits > TW_MAX_LOG) return set_error(ZKGPU_ERR_ARG, "lagrange_xi_rows: bits");
    const uint64_t N = 1ULL << n_bits;
    if (row0 > N || nrows > N - row0 || (nrows && ld < nrows))
        return set_error(ZKGPU_ERR_ARG, "lagrange_xi_rows: rows [%llu, +%llu) outside the domain or ld too small",
                         (unsigned long long)row0, (unsigned long long)nrows);
    const uint64_t x[3] = {xi[0] % ZK_P, xi[1] % ZK_P, xi[2] % ZK_P};
    if (x[1] == 0 && x[2] == 0)  // xi in the base field: x_k - xi may vanish; the caller interpolates instead
        return set_error(ZKGPU_ERR_ARG, "lagrange_xi_rows: xi lies in the base field");
    // scale = (1 - xi^N) / N
    uint64_t p[3] = {1, 0, 0}, b[3] = {x[0], x[1], x[2]};
    for (uint64_t e = N; e; e >>= 1) {
        if (e & 1) h3_mul(p, p, b);
        h3_mul(b, b, b);
    }
    const uint64_t ninv = h_inv(N % ZK_P);
    const uint64_t scale[3] = {h_mul((1 + ZK_P - p[0]) % ZK_P, ninv), h_mul((ZK_P - p[1]) % ZK_P, ninv),
                               h_mul((ZK_P - p[2]) % ZK_P, ninv)};
    const uint64_t w = h_w(n_bits);
    const uint64_t wx[3] = {h_mul(x[0], w), h_mul(x[1], w), h_mul(x[2], w)};
    return xdiv_rows(lev, lpev, ld, 0, x, wx, 1, scale, n_bits, row0, nrows, g_ctx.stream);
}

int zkgpu_ext_powers_dev(uint64_t *out, uint64_t ld, const uint64_t base[3], uint64_t n)
{
    int rc;
    if ((rc = require_init())) return rc;
    if (!n) return 0;
    if (ld < n) return set_error(ZKGPU_ERR_ARG, "ext_powers: ld < n");
    return ext_powers(out, ld, base, n, g_ctx.stream);
}

int zkgpu_scale_by_powers_dev(uint64_t *cols, uint64_t ld, uint32_t ncols, uint64_t n, uint64_t base)
{
    int rc;
    if ((rc = require_init())) return rc;
    if (!n || !ncols) return 0;
    if (ld < n) return set_error(ZKGPU_ERR_ARG, "scale_by_powers: ld < n");
    return scale_powers(cols, ld, ncols, n, base, g_ctx.stream);
}

int zkgpu_qsplit_dev(uint64_t *qq2, uint64_t ld2, const uint64_t *qq1, uint64_t ld1, uint64_t n, uint32_t q_deg,
                     uint64_t shift_in)
{
    int rc;
    if ((rc = require_init())) return rc;
    if (!n) return 0;
    if (ld2 < n || ld1 / n < q_deg) return set_error(ZKGPU_ERR_ARG, "qsplit: ld2 < n or ld1 < q_deg * n");
    return qsplit(qq2, ld2, qq1, ld1, n, q_deg, shift_in, 3, 3, g_ctx.stream);
}

int zkgpu_qsplit_cols_dev(uint64_t *qq2, uint64_t ld2, const uint64_t *qq1, uint64_t ld1, uint64_t n, uint32_t q_deg,
                          uint64_t shift_in, uint32_t dim, uint32_t stride)
{
    int rc;
    if ((rc = require_init())) return rc;
    if (!n || !dim) return 0;
    if (dim > stride) return set_error(ZKGPU_ERR_ARG, "qsplit_cols: dim %u > stride %u", dim, stride);
    if (ld2 < n || ld1 / n < q_deg) return set_error(ZKGPU_ERR_ARG, "qsplit_cols: ld2 < n or ld1 < q_deg * n");
    return qsplit(qq2, ld2, qq1, ld1, n, q_deg, shift_in, dim, stride, g_ctx.stream);
}

int zkgpu_h1h2_dev(uint64_t *h1, uint64_t h1_ld, uint64_t *h2, uint64_t h2_ld, const uint64_t *f, uint64_t f_ld,
                   const uint64_t *t, uint64_t t_ld, uint64_t n, uint32_t dim, uint64_t *missing_row)
{
    int rc;
    if (missing_row) *missing_row = ~0ULL;
    if ((rc = require_init())) return rc;
    if (dim != 1 && dim != 3) return set_error(ZKGPU_ERR_ARG, "h1h2: dim must be 1 or 3");
    if (n > 0x7FFFFFFFULL) return set_error(ZKGPU_ERR_ARG, "h1h2: n too large");
    if (dim == 3 && (h1_ld < n || h2_ld < n || f_ld < n || t_ld < n))
        return set_error(ZKGPU_ERR_ARG, "h1h2: ld < n");
    if (!n) return 0;
    return h1h2(h1, h1_ld, h2, h2_ld, f, f_ld, t, t_ld, n, dim, missing_row, g_ctx.stream);
}

// ---- calculateH1H2 over row-sharded f / t (include/zkgpu.h)
static int h1h2_shard_args(uint32_t dim, uint64_t n)
{
    if (dim != 1 && dim != 3) return set_error(ZKGPU_ERR_ARG, "h1h2 (sharded): dim must be 1 or 3");
    if (n > 0x7FFFFFFFULL) return set_error(ZKGPU_ERR_ARG, "h1h2 (sharded): n too large");
    return 0;
}

int zkgpu_h1h2_shard_route(uint64_t *recs, uint64_t cap, uint32_t *n_t, uint32_t *n_f, const uint64_t *f,
                           uint64_t f_ld, const uint64_t *t, uint64_t t_ld, uint64_t nrows, uint64_t row0, uint32_t dim,
                           uint32_t world)
{
    int rc;
    if ((rc = require_init()) || (rc = h1h2_shard_args(dim, nrows))) return rc;
    if (!world || !nrows) return set_error(ZKGPU_ERR_ARG, "h1h2 (sharded): empty world or block");
    if (f_ld < nrows || t_ld < nrows) return set_error(ZKGPU_ERR_ARG, "h1h2 (sharded): ld < nrows");
    if (row0 + nrows > 0xFFFFFFFFULL) return set_error(ZKGPU_ERR_ARG, "h1h2 (sharded): rows beyond 2^32");
    return h1h2_shard_route(recs, cap, n_t, n_f, f, f_ld, t, t_ld, nrows, row0, dim, world, g_ctx.stream);
}

int zkgpu_h1h2_shard_owner(uint64_t *ret, const uint64_t *recs, uint64_t nrec, uint32_t dim, uint64_t *missing_row)
{
    int rc;
    *missing_row = ~0ULL;
    if ((rc = require_init()) || (rc = h1h2_shard_args(dim, nrec))) return rc;
    return h1h2_shard_owner(ret, recs, nrec, dim, missing_row, g_ctx.stream);
}

int zkgpu_h1h2_shard_counts(uint32_t *start, uint32_t *cnt, uint64_t *total, const uint64_t *sent, const uint64_t *ret,
                            uint64_t nsent, uint64_t nrows, uint64_t row0)
{
    int rc;
    if ((rc = require_init()) || (rc = h1h2_shard_args(1, nrows))) return rc;
    if (!nrows) return set_error(ZKGPU_ERR_ARG, "h1h2 (sharded): empty block");
    return h1h2_shard_counts(start, cnt, total, sent, ret, nsent, nrows, row0, g_ctx.stream);
}

int zkgpu_h1h2_shard_deal(uint64_t *seg, uint64_t seg_ld, const uint64_t *t, uint64_t t_ld, const uint32_t *start,
                          const uint32_t *cnt, uint64_t nrows, uint32_t dim)
{
    int rc;
    if ((rc = require_init()) || (rc = h1h2_shard_args(dim, nrows))) return rc;
    if (!nrows) return 0;
    return h1h2_shard_deal(seg, seg_ld, t, t_ld, start, cnt, nrows, dim, g_ctx.stream);
}

int zkgpu_h1h2_shard_place(uint64_t *h1, uint64_t h1_ld, uint64_t *h2, uint64_t h2_ld, const uint64_t *buf,
                           uint64_t buf_ld, uint64_t pos0, uint64_t len, uint64_t row0, uint32_t dim)
{
    int rc;
    if ((rc = require_init()) || (rc = h1h2_shard_args(dim, len))) return rc;
    if (len && (pos0 >> 1) < row0) return set_error(ZKGPU_ERR_ARG, "h1h2 (sharded): position before the block");
    return h1h2_shard_place(h1, h1_ld, h2, h2_ld, buf, buf_ld, pos0, len, row0, dim, g_ctx.stream);
}

int zkgpu_cols3_to_interleaved_dev(uint64_t *out, const uint64_t *cols, uint64_t ld, uint64_t n)
{
    int rc;
    if ((rc = require_init())) return rc;
    if (!n) return 0;
    if (ld < n) return set_error(ZKGPU_ERR_ARG, "cols3_to_interleaved: ld < n");
    return cols3_to_interleaved(out, cols, ld, n, g_ctx.stream);
}

int zkgpu_gl_merkle_open_rows_dev(uint64_t *vals_out, uint64_t *sibs_out, const uint64_t *nodes, const uint64_t *src,
                                  uint64_t ncols, uint64_t nrows, const uint64_t *idx, uint64_t nq)
{
    int rc;
    if ((rc = require_init())) return rc;
    if (!nq) return 0;
    Ctx &c = g_ctx;
    if (nrows == 0 || (nrows & (nrows - 1)))
        return set_error(ZKGPU_ERR_ARG, "merkle_open_rows: nrows %llu is not a power of two", (unsigned long long)nrows);
    uint32_t nlev = log2u(nrows);
    for (uint64_t q = 0; q < nq; q++)
        if (idx[q] >= nrows)
            return set_error(ZKGPU_ERR_ARG, "merkle_open_rows: index %llu >= nrows", (unsigned long long)idx[q]);
    size_t nv = nq * ncols, ns = nq * nlev * 4;
    uint64_t *d = workspace(2, (nq + nv + ns + 1) * sizeof(uint64_t));
    if (!d) return ZKGPU_ERR_OOM;
    uint64_t *didx = d, *dv = d + nq, *ds = d + nq + nv;
    if ((rc = check_hip(hipMemcpyAsync(didx, idx, nq * 8, hipMemcpyHostToDevice, c.stream), "H2D"))) return rc;
    if ((rc = merkle_open_strided(dv, ds, nodes, src, ncols, nrows, ncols, 1, didx, nq, c.stream))) return rc;
    if (nv && (rc = check_hip(hipMemcpyAsync(vals_out, dv, nv * 8, hipMemcpyDeviceToHost, c.stream), "D2H"))) return rc;
    if (ns && (rc = check_hip(hipMemcpyAsync(sibs_out, ds, ns * 8, hipMemcpyDeviceToHost, c.stream), "D2H"))) return rc;
    return check_hip(hipStreamSynchronize(c.stream), "merkle_open_rows sync");
}

// all query openings of a proof in one round trip: [indices of every request |
// vals, sibs of every request] in workspace 2, mirrored in a page-locked host
// buffer so that the upload and the download are one copy each
int zkgpu_gl_merkle_open_many(const zkgpu_open_req *req, uint32_t n)
{
    int rc;
    if ((rc = require_init())) return rc;
    Ctx &c = g_ctx;
    uint64_t ni = 0, no = 0;
    for (uint32_t k = 0; k < n; k++) {
        const zkgpu_open_req &r = req[k];
        if (r.nrows == 0 || (r.nrows & (r.nrows - 1)))
            return set_error(ZKGPU_ERR_ARG, "merkle_open_many: request %u: nrows %llu is not a power of two", k,
                             (unsigned long long)r.nrows);
        for (uint64_t q = 0; q < r.nq; q++)
            if (r.idx[q] >= r.nrows)
                return set_error(ZKGPU_ERR_ARG, "merkle_open_many: request %u: index %llu >= nrows", k,
                                 (unsigned long long)r.idx[q]);
        ni += r.nq;
        no += r.nq * (r.ncols + log2u(r.nrows) * 4ULL);
    }
    if (!ni) return 0;
    static uint64_t *pin = nullptr;
    static uint64_t pin_words = 0;
    if (pin_words < ni + no) {
        if (pin) (void)hipHostFree(pin);
        pin = nullptr;
        pin_words = 0;
        if ((rc = check_hip(hipHostMalloc((void **)&pin, (ni + no) * 8, hipHostMallocDefault), "open_many pin")))
            return rc;
        pin_words = ni + no;
    }
    uint64_t *d = workspace(2, (ni + no) * 8);
    if (!d) return ZKGPU_ERR_OOM;
    for (uint32_t k = 0, i = 0; k < n; i += req[k].nq, k++) memcpy(pin + i, req[k].idx, req[k].nq * 8);
    if ((rc = check_hip(hipMemcpyAsync(d, pin, ni * 8, hipMemcpyHostToDevice, c.stream), "open_many H2D"))) return rc;
    uint64_t io = 0, oo = ni;
    for (uint32_t k = 0; k < n; k++) {
        const zkgpu_open_req &r = req[k];
        if (!r.nq) continue;
        uint64_t *dv = d + oo, *ds = dv + r.nq * r.ncols;
        rc = r.rows ? merkle_open_strided(dv, ds, r.nodes, r.src, r.ncols, r.nrows, r.ncols, 1, d + io, r.nq, c.stream)
                    : merkle_open_cols(dv, ds, r.nodes, r.src, r.ncols, r.nrows, r.ld, d + io, r.nq, c.stream);
        if (rc) return rc;
        io += r.nq;
        oo += r.nq * (r.ncols + log2u(r.nrows) * 4ULL);
    }
    if ((rc = check_hip(hipMemcpyAsync(pin + ni, d + ni, no * 8, hipMemcpyDeviceToHost, c.stream), "open_many D2H")))
        return rc;
    if ((rc = check_hip(hipStreamSynchronize(c.stream), "open_many sync"))) return rc;
    oo = ni;
    for (uint32_t k = 0; k < n; k++) {
        const zkgpu_open_req &r = req[k];
        const uint64_t nv = r.nq * r.ncols, ns = r.nq * log2u(r.nrows) * 4ULL;
        if (nv) memcpy(r.vals_out, pin + oo, nv * 8);
        if (ns) memcpy(r.sibs_out, pin + oo + nv, ns * 8);
        oo += nv + ns;
    }
    return 0;
}

// ---------------------------------------------------------------- FRI
int zkgpu_fri_fold_dev(uint64_t *out, const uint64_t *pol, uint32_t pol_bits, uint32_t out_bits,
                       const uint64_t special_x[3], uint64_t shift_inv)
{
    int rc;
    if ((rc = require_init())) return rc;
    return fri_fold(out, pol, pol_bits, out_bits, special_x, shift_inv, g_ctx.stream);
}

int zkgpu_fri_fold_rows_dev(uint64_t *out, const uint64_t *rows, uint64_t g0, uint64_t ngroups, uint32_t pol_bits,
                            uint32_t out_bits, const uint64_t special_x[3], uint64_t shift_inv)
{
    int rc;
    if ((rc = require_init())) return rc;
    return fri_fold_rows(out, rows, g0, ngroups, pol_bits, out_bits, special_x, shift_inv, g_ctx.stream);
}

int zkgpu_fri_transpose_dev(uint64_t *aux, const uint64_t *pol, uint64_t degree, uint32_t transpose_bits)
{
    int rc;
    if ((rc = require_init())) return rc;
    return fri_transpose(aux, pol, degree, transpose_bits, g_ctx.stream);
}

}  // extern "C"

// ---------------------------------------------------------------- profiling
#include <string>
#include <vector>

namespace zk {
struct ProfRec {
    std::string name;
    hipEvent_t start, stop;
    double bytes;
};
static bool g_prof = false;
static std::vector<ProfRec> g_prof_recs;
static std::vector<hipEvent_t> g_event_pool;
static hipEvent_t g_pending_start = nullptr;

static hipEvent_t get_event()
{
    if (!g_event_pool.empty()) {
        hipEvent_t e = g_event_pool.back();
        g_event_pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}

bool prof_on() { return g_prof; }

void prof_begin(hipStream_t s)
{
    if (!g_prof) return;
    g_pending_start = get_event();
    (void)hipEventRecord(g_pending_start, s);
}

void prof_end(const char *kernel, double bytes, hipStream_t s)
{
    if (!g_prof || !g_pending_start) return;
    hipEvent_t stop = get_event();
    (void)hipEventRecord(stop, s);
    g_prof_recs.push_back(ProfRec{kernel, g_pending_start, stop, bytes});
    g_pending_start = nullptr;
}
}  // namespace zk

extern "C" {
int zkgpu_prof_enable(int on)
{
    zk::g_prof = on != 0;
    return 0;
}

int zkgpu_prof_reset(void)
{
    (void)hipStreamSynchronize(zk::g_ctx.stream);
    for (auto &r : zk::g_prof_recs) {
        zk::g_event_pool.push_back(r.start);
        zk::g_event_pool.push_back(r.stop);
    }
    zk::g_prof_recs.clear();
    return 0;
}

int zkgpu_prof_query(const char *kernel, uint64_t *launches, double *total_ms, double *total_bytes)
{
    int rc;
    if ((rc = zk::check_hip(hipStreamSynchronize(zk::g_ctx.stream), "prof sync"))) return rc;
    uint64_t n = 0;
    double ms = 0, bytes = 0;
    for (auto &r : zk::g_prof_recs) {
        if (r.name != kernel) continue;
        float t = 0;
        if ((rc = zk::check_hip(hipEventSynchronize(r.stop), "prof event"))) return rc;
        if ((rc = zk::check_hip(hipEventElapsedTime(&t, r.start, r.stop), "prof elapsed"))) return rc;
        n++;
        ms += t;
        bytes += r.bytes;
    }
    *launches = n;
    *total_ms = ms;
    *total_bytes = bytes;
    return 0;
}

int zkgpu_prof_kernels(char *buf, uint64_t buflen)
{
    std::vector<std::string> seen;
    for (auto &r : zk::g_prof_recs) {
        bool dup = false;
        for (auto &s : seen) dup |= (s == r.name);
        if (!dup) seen.push_back(r.name);
    }
    std::string out;
    for (auto &s : seen) out += s + "\n";
    if (buflen == 0) return 0;
    size_t n = out.size() < buflen - 1 ? out.size() : buflen - 1;
    memcpy(buf, out.data(), n);
    buf[n] = 0;
    return 0;
}
// stream marks for the host prover's stage timers (no synchronisation);
// events belong to a device: a zkgpu_init on another device drops them
static hipEvent_t g_marks[ZKGPU_MARKS];
static int g_marks_dev = -1;
int zkgpu_mark(uint32_t slot)
{
    int rc;
    if ((rc = require_init())) return rc;
    if (slot >= ZKGPU_MARKS) return set_error(ZKGPU_ERR_ARG, "mark: slot %u >= %d", slot, ZKGPU_MARKS);
    if (g_marks_dev != g_ctx.device) {
        for (hipEvent_t &e : g_marks)
            if (e) {
                (void)hipEventDestroy(e);
                e = nullptr;
            }
        g_marks_dev = g_ctx.device;
    }
    if (!g_marks[slot] && (rc = check_hip(hipEventCreate(&g_marks[slot]), "mark event"))) return rc;
    return check_hip(hipEventRecord(g_marks[slot], g_ctx.stream), "mark record");
}
int zkgpu_mark_elapsed(uint32_t a, uint32_t b, double *ms)
{
    int rc;
    if (a >= ZKGPU_MARKS || b >= ZKGPU_MARKS || !g_marks[a] || !g_marks[b] || !ms)
        return set_error(ZKGPU_ERR_ARG, "mark_elapsed: slots %u / %u not recorded", a, b);
    if ((rc = check_hip(hipEventSynchronize(g_marks[b]), "mark sync"))) return rc;
    float t = 0;
    if ((rc = check_hip(hipEventElapsedTime(&t, g_marks[a], g_marks[b]), "mark elapsed"))) return rc;
    *ms = t;
    return 0;
}
}  // extern "C"
