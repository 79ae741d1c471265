// Plookup h1/h2 columns on the GPU: Polinomial::calculateH1H2_opt1 (dim 1,
// polinomial.hpp:349-463) / calculateH1H2_opt3 (dim 3, :465-583), called per
// plookup from Starks::genProof stage 2 (starks.cpp:104-127).
//
// The reference builds a chained hash table of the table column t (each key
// remembers its LAST row), counts every f value onto that row, and deals the
// resulting multiset (t[j] repeated 1 + count_j times, in t order) alternately
// into h1 and h2.  The same mapping, data-parallel (h1h2_hash): an
// open-addressing table of table ROWS keyed by the canonical value (linear
// probing, 2^k >= 2N slots of u32): insertion keeps the largest row per key
// (atomicMax: the reference's "last row wins"), every f row probes and counts
// onto its row (counts start at 1; an absent key records the smallest such f
// row, "Number not included"), an exclusive scan of the counts gives each
// table row its start in the 2N-long multiset, and one thread per table row
// scatters its 1 + count raw copies (copyElement) alternately into h1 / h2.
// Columns are column-major: component c of a dim-3 column at ptr + c * ld.
// (A stable radix sort of the keys with a two-level upper_bound was the
// round-2 form: 8.1 against 1.9 ms for two plookups at 2^23.)
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include <rocprim/device/device_scan.hpp>

#include "gl_device.hpp"
#include "zkgpu_internal.hpp"

namespace zk {

static inline uint32_t nblk2(uint64_t n, uint32_t t) { return (uint32_t)((n + t - 1) / t); }

__global__ void k_h12_fill1(uint32_t *c, uint64_t n)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) c[i] = 1;
}

// ---------------------------------------------------------------- hash path
constexpr uint32_t H12_EMPTY = 0xFFFFFFFFu;

template <int DIM>
__device__ __forceinline__ void h12_key(uint64_t key[DIM], const uint64_t *col, uint64_t ld, uint64_t r)
{
#pragma unroll
    for (int c = 0; c < DIM; c++) key[c] = gl_canon(col[c * ld + r]);
}

template <int DIM>
__device__ __forceinline__ uint64_t h12_hash(const uint64_t key[DIM])
{
    uint64_t h = 0x9E3779B97F4A7C15ULL;
#pragma unroll
    for (int c = 0; c < DIM; c++) {
        uint64_t z = key[c] + h;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
        h = z ^ (z >> 31);
    }
    return h;
}

template <int DIM>
__device__ __forceinline__ bool h12_eq(const uint64_t *t, uint64_t t_ld, uint32_t row, const uint64_t key[DIM])
{
#pragma unroll
    for (int c = 0; c < DIM; c++)
        if (gl_canon(t[c * t_ld + row]) != key[c]) return false;
    return true;
}

// table row i -> its key's slot holds the largest row with that key
template <int DIM>
__global__ void __launch_bounds__(256) k_h12_insert(uint32_t *slots, uint64_t mask, const uint64_t *t, uint64_t t_ld,
                                                    uint64_t n)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t key[DIM];
    h12_key<DIM>(key, t, t_ld, i);
    uint64_t h = h12_hash<DIM>(key) & mask;
    for (uint64_t probe = 0; probe <= mask; probe++, h = (h + 1) & mask) {
        uint32_t cur = slots[h];
        if (cur == H12_EMPTY) {
            cur = atomicCAS(&slots[h], H12_EMPTY, (uint32_t)i);
            if (cur == H12_EMPTY) return;
        }
        if (h12_eq<DIM>(t, t_ld, cur, key)) {
            atomicMax(&slots[h], (uint32_t)i);
            return;
        }
    }
}

// f row i -> ++cnt[last table row with f's key]; absent keys record the
// smallest such row
template <int DIM>
__global__ void __launch_bounds__(256) k_h12_probe(const uint32_t *slots, uint64_t mask, const uint64_t *f,
                                                   uint64_t f_ld, const uint64_t *t, uint64_t t_ld, uint64_t n,
                                                   uint32_t *cnt, unsigned long long *miss)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t key[DIM];
    h12_key<DIM>(key, f, f_ld, i);
    uint64_t h = h12_hash<DIM>(key) & mask;
    for (uint64_t probe = 0; probe <= mask; probe++, h = (h + 1) & mask) {
        const uint32_t cur = slots[h];
        if (cur == H12_EMPTY) break;
        if (h12_eq<DIM>(t, t_ld, cur, key)) {
            atomicAdd(&cnt[cur], 1u);
            return;
        }
    }
    atomicMin(miss, (unsigned long long)i);
}

// table row j: its 1 + count copies at multiset slots start[j] ..
template <int DIM>
__global__ void __launch_bounds__(256) k_h12_scatter(uint64_t *h1, uint64_t h1_ld, uint64_t *h2, uint64_t h2_ld,
                                                     const uint64_t *t, uint64_t t_ld, const uint32_t *start,
                                                     const uint32_t *cnt, uint64_t n)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    uint64_t v[DIM];
#pragma unroll
    for (int c = 0; c < DIM; c++) v[c] = t[c * t_ld + j];  // raw copy (copyElement)
    const uint64_t s0 = start[j], e = s0 + cnt[j];
    for (uint64_t sl = s0; sl < e; sl++) {
        uint64_t *h = (sl & 1) ? h2 : h1;
        const uint64_t ld = (sl & 1) ? h2_ld : h1_ld;
#pragma unroll
        for (int c = 0; c < DIM; c++) h[c * ld + (sl >> 1)] = v[c];
    }
}

static int h1h2_hash(uint64_t *h1, uint64_t h1_ld, uint64_t *h2, uint64_t h2_ld, const uint64_t *f, uint64_t f_ld,
                     const uint64_t *t, uint64_t t_ld, uint64_t n, uint32_t dim, uint64_t *missing_row, hipStream_t s)
{
    uint64_t m = 1;
    while (m < 2 * n) m <<= 1;
    const size_t need = m * 4 + 2 * n * 4 + 16;
    char *w = (char *)workspace(4, need);
    if (!w) return ZKGPU_ERR_OOM;
    uint32_t *slots = (uint32_t *)w;
    uint32_t *cnt = slots + m;
    uint32_t *start = cnt + n;
    unsigned long long *miss = (unsigned long long *)(((uintptr_t)(start + n) + 7) & ~(uintptr_t)7);
    size_t scan_bytes = 0;
    if (rocprim::exclusive_scan(nullptr, scan_bytes, cnt, start, 0u, (size_t)n, rocprim::plus<uint32_t>(), s) !=
        hipSuccess)
        return set_error(ZKGPU_ERR_HIP, "h1h2: rocprim temp-size query failed");
    void *tmp = workspace(5, scan_bytes);
    if (!tmp) return ZKGPU_ERR_OOM;
    const uint32_t B = 256;
    prof_begin(s);
    if (check_hip(hipMemsetAsync(slots, 0xFF, m * 4, s), "h1h2 memset") ||
        check_hip(hipMemsetAsync(miss, 0xFF, 8, s), "h1h2 memset"))
        return ZKGPU_ERR_HIP;
    hipLaunchKernelGGL(k_h12_fill1, dim3(nblk2(n, B)), dim3(B), 0, s, cnt, n);
    if (dim == 1) {
        hipLaunchKernelGGL(k_h12_insert<1>, dim3(nblk2(n, B)), dim3(B), 0, s, slots, m - 1, t, t_ld, n);
        hipLaunchKernelGGL(k_h12_probe<1>, dim3(nblk2(n, B)), dim3(B), 0, s, slots, m - 1, f, f_ld, t, t_ld, n, cnt,
                           miss);
    } else {
        hipLaunchKernelGGL(k_h12_insert<3>, dim3(nblk2(n, B)), dim3(B), 0, s, slots, m - 1, t, t_ld, n);
        hipLaunchKernelGGL(k_h12_probe<3>, dim3(nblk2(n, B)), dim3(B), 0, s, slots, m - 1, f, f_ld, t, t_ld, n, cnt,
                           miss);
    }
    {
        size_t tb = scan_bytes;
        if (rocprim::exclusive_scan(tmp, tb, cnt, start, 0u, (size_t)n, rocprim::plus<uint32_t>(), s) != hipSuccess)
            return set_error(ZKGPU_ERR_HIP, "h1h2: scan failed");
    }
    unsigned long long mh = 0;
    if (check_hip(hipMemcpyAsync(&mh, miss, 8, hipMemcpyDeviceToHost, s), "D2H") ||
        check_hip(hipStreamSynchronize(s), "h1h2 sync"))
        return ZKGPU_ERR_HIP;
    if (mh != ~0ULL) {
        if (missing_row) *missing_row = mh;
        return set_error(ZKGPU_ERR_ARG, "calculateH1H2: Number not included: w=%llu", mh);
    }
    if (missing_row) *missing_row = ~0ULL;
    if (dim == 1)
        hipLaunchKernelGGL(k_h12_scatter<1>, dim3(nblk2(n, B)), dim3(B), 0, s, h1, h1_ld, h2, h2_ld, t, t_ld, start, cnt,
                           n);
    else
        hipLaunchKernelGGL(k_h12_scatter<3>, dim3(nblk2(n, B)), dim3(B), 0, s, h1, h1_ld, h2, h2_ld, t, t_ld, start, cnt,
                           n);
    prof_end("k_h1h2", (double)dim * 8.0 * 4.0 * n, s);
    return check_launch("h1h2");
}

int h1h2(uint64_t *h1, uint64_t h1_ld, uint64_t *h2, uint64_t h2_ld, const uint64_t *f, uint64_t f_ld,
         const uint64_t *t, uint64_t t_ld, uint64_t n, uint32_t dim, uint64_t *missing_row, hipStream_t s)
{
    return h1h2_hash(h1, h1_ld, h2, h2_ld, f, f_ld, t, t_ld, n, dim, missing_row, s);
}

// ---------------------------------------------------------------- row-sharded
// calculateH1H2 over W ranks, each holding rows [row0, row0 + n) of f and t
// (host/sharded_starks.hpp h1h2_all).  The mapping is the one above: table
// row j appears 1 + count_j times in the multiset (count_j = the f rows with
// t[j]'s key, on the LAST table row with that key, else 0), in table order,
// dealt alternately into h1 / h2.  Split as:
//   route   each rank dedupes its rows: distinct t keys with their largest
//           row, distinct f keys with their count and smallest row; each
//           distinct key goes to the rank owning hash(key) as a record
//           {k0, k1, k2, global row, val} (val = H12S_T for a t key, the f
//           count otherwise), bucketed by owner, t records first
//   owner   per key: the largest t row over all ranks, the f counts summed;
//           f keys with no t row give the smallest such f row (the
//           reference's "Number not included"); returns, aligned with the t
//           records, the count for the winning row (0 for the others)
//   counts  the sender: count_j = 1 + returned count of row j; exclusive
//           scan -> the rank's multiset positions, relative to its offset
//   deal    the rank's segment of the multiset (its table rows' copies)
//   place   a received piece of the multiset into the rank's h1 / h2 rows
constexpr uint64_t H12S_T = ~0ULL;
constexpr int H12S_REC = 5;  // words per record

__device__ __forceinline__ uint32_t h12s_owner(uint64_t h, uint32_t world)
{
    return (uint32_t)(((h >> 32) * (uint64_t)world) >> 32);  // high hash bits (the table probes use the low ones)
}

// local f table: slot -> smallest row with the key, fcnt[slot] = its rows
template <int DIM>
__global__ void __launch_bounds__(256) k_h12s_insert_f(uint32_t *slots, uint32_t *fcnt, uint64_t mask,
                                                       const uint64_t *f, uint64_t f_ld, uint64_t n)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t key[DIM];
    h12_key<DIM>(key, f, f_ld, i);
    uint64_t h = h12_hash<DIM>(key) & mask;
    for (uint64_t probe = 0; probe <= mask; probe++, h = (h + 1) & mask) {
        uint32_t cur = slots[h];
        if (cur == H12_EMPTY) {
            cur = atomicCAS(&slots[h], H12_EMPTY, (uint32_t)i);
            if (cur == H12_EMPTY) {
                atomicAdd(&fcnt[h], 1u);
                return;
            }
        }
        if (h12_eq<DIM>(f, f_ld, cur, key)) {  // every row a slot ever holds has its key
            atomicMin(&slots[h], (uint32_t)i);
            atomicAdd(&fcnt[h], 1u);
            return;
        }
    }
}

// records of the occupied slots of the local t table (tab 0) and f table
// (tab 1): count per owner (pass 0) or write into the owner's bucket (pass 1)
template <int DIM>
__global__ void __launch_bounds__(256) k_h12s_bucket(uint64_t *recs, const uint32_t *tslots, const uint32_t *fslots,
                                                     const uint32_t *fcnt, uint64_t m, const uint64_t *t, uint64_t t_ld,
                                                     const uint64_t *f, uint64_t f_ld, uint64_t row0, uint32_t world,
                                                     uint32_t *cnt /* 2 W */, const uint64_t *base /* 2 W */,
                                                     int pass)
{
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= 2 * m) return;
    const int tab = k >= m;
    const uint64_t sl = tab ? k - m : k;
    const uint32_t row = tab ? fslots[sl] : tslots[sl];
    if (row == H12_EMPTY) return;
    uint64_t key[DIM];
    h12_key<DIM>(key, tab ? f : t, tab ? f_ld : t_ld, row);
    const uint32_t o = h12s_owner(h12_hash<DIM>(key), world);
    const uint32_t pos = atomicAdd(&cnt[2 * o + tab], 1u);
    if (!pass) return;
    uint64_t *r = recs + (base[2 * o + tab] + pos) * H12S_REC;
#pragma unroll
    for (int c = 0; c < 3; c++) r[c] = c < DIM ? key[c] : 0;
    r[3] = row0 + row;
    r[4] = tab ? (uint64_t)fcnt[sl] : H12S_T;
}

template <int DIM>
__device__ __forceinline__ void h12s_rkey(uint64_t key[DIM], const uint64_t *r)
{
#pragma unroll
    for (int c = 0; c < DIM; c++) key[c] = r[c];
}

template <int DIM>
__device__ __forceinline__ bool h12s_req(const uint64_t *r, const uint64_t key[DIM])
{
#pragma unroll
    for (int c = 0; c < DIM; c++)
        if (r[c] != key[c]) return false;
    return true;
}

// owner: t records -> slot = ((row + 1) << 32 | record), largest row wins
template <int DIM>
__global__ void __launch_bounds__(256) k_h12s_own_insert(unsigned long long *slots, uint64_t mask, const uint64_t *recs,
                                                         uint64_t nrec)
{
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nrec) return;
    const uint64_t *r = recs + k * H12S_REC;
    if (r[4] != H12S_T) return;
    uint64_t key[DIM];
    h12s_rkey<DIM>(key, r);
    const unsigned long long mine = ((unsigned long long)(r[3] + 1) << 32) | k;
    uint64_t h = h12_hash<DIM>(key) & mask;
    for (uint64_t probe = 0; probe <= mask; probe++, h = (h + 1) & mask) {
        unsigned long long cur = slots[h];
        if (!cur) {
            cur = atomicCAS(&slots[h], 0ULL, mine);
            if (!cur) return;
        }
        if (h12s_req<DIM>(recs + (cur & 0xFFFFFFFFULL) * H12S_REC, key)) {
            atomicMax(&slots[h], mine);
            return;
        }
    }
}

template <int DIM>
__device__ __forceinline__ uint64_t h12s_find(const unsigned long long *slots, uint64_t mask, const uint64_t *recs,
                                              const uint64_t key[DIM])
{
    uint64_t h = h12_hash<DIM>(key) & mask;
    for (uint64_t probe = 0; probe <= mask; probe++, h = (h + 1) & mask) {
        const unsigned long long cur = slots[h];
        if (!cur) break;
        if (h12s_req<DIM>(recs + (cur & 0xFFFFFFFFULL) * H12S_REC, key)) return cur & 0xFFFFFFFFULL;
    }
    return ~0ULL;
}

// owner: f records -> the winning t record's sum; absent keys: smallest row
template <int DIM>
__global__ void __launch_bounds__(256) k_h12s_own_probe(const unsigned long long *slots, uint64_t mask,
                                                        const uint64_t *recs, uint64_t nrec,
                                                        unsigned long long *sum, unsigned long long *miss)
{
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nrec) return;
    const uint64_t *r = recs + k * H12S_REC;
    if (r[4] == H12S_T) return;
    uint64_t key[DIM];
    h12s_rkey<DIM>(key, r);
    const uint64_t w = h12s_find<DIM>(slots, mask, recs, key);
    if (w == ~0ULL)
        atomicMin(miss, (unsigned long long)r[3]);
    else
        atomicAdd(&sum[w], (unsigned long long)r[4]);
}

// owner: the return value of each t record (its count if it won its key)
template <int DIM>
__global__ void __launch_bounds__(256) k_h12s_own_ret(uint64_t *ret, const unsigned long long *slots, uint64_t mask,
                                                      const uint64_t *recs, uint64_t nrec,
                                                      const unsigned long long *sum)
{
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nrec) return;
    const uint64_t *r = recs + k * H12S_REC;
    if (r[4] != H12S_T) {
        ret[k] = 0;
        return;
    }
    uint64_t key[DIM];
    h12s_rkey<DIM>(key, r);
    ret[k] = h12s_find<DIM>(slots, mask, recs, key) == k ? sum[k] : 0;
}

// sender: count_j = 1 + the count returned for row j's record
__global__ void k_h12s_apply(uint32_t *cnt, const uint64_t *sent, const uint64_t *ret, uint64_t nsent, uint64_t row0)
{
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nsent) return;
    const uint64_t *r = sent + k * H12S_REC;
    if (r[4] == H12S_T && ret[k]) cnt[r[3] - row0] += (uint32_t)ret[k];  // one record per row: no race
}

// the rank's multiset segment: table row j's copies at start[j] .. (raw, like copyElement)
template <int DIM>
__global__ void __launch_bounds__(256) k_h12s_deal(uint64_t *seg, uint64_t seg_ld, const uint64_t *t, uint64_t t_ld,
                                                   const uint32_t *start, const uint32_t *cnt, uint64_t n)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    uint64_t v[DIM];
#pragma unroll
    for (int c = 0; c < DIM; c++) v[c] = t[c * t_ld + j];
    const uint64_t s0 = start[j], e = s0 + cnt[j];
    for (uint64_t p = s0; p < e; p++)
#pragma unroll
        for (int c = 0; c < DIM; c++) seg[c * seg_ld + p] = v[c];
}

// multiset positions [pos0, pos0 + len) (buf column-major, ld buf_ld) ->
// h1 (even positions) / h2 (odd) at local row p / 2 - row0
template <int DIM>
__global__ void __launch_bounds__(256) k_h12s_place(uint64_t *h1, uint64_t h1_ld, uint64_t *h2, uint64_t h2_ld,
                                                    const uint64_t *buf, uint64_t buf_ld, uint64_t pos0, uint64_t len,
                                                    uint64_t row0)
{
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= len) return;
    const uint64_t p = pos0 + k;
    uint64_t *h = (p & 1) ? h2 : h1;
    const uint64_t ld = (p & 1) ? h2_ld : h1_ld;
#pragma unroll
    for (int c = 0; c < DIM; c++) h[c * ld + (p >> 1) - row0] = buf[c * buf_ld + k];
}

static uint64_t h12s_table_size(uint64_t n)
{
    uint64_t m = 1;
    while (m < 2 * n) m <<= 1;
    return m;
}

int h1h2_shard_route(uint64_t *recs, uint64_t cap, uint32_t *n_t, uint32_t *n_f, const uint64_t *f, uint64_t f_ld,
                     const uint64_t *t, uint64_t t_ld, uint64_t n, uint64_t row0, uint32_t dim, uint32_t world,
                     hipStream_t s)
{
    const uint64_t m = h12s_table_size(n);
    const size_t need = 3 * m * 4 + 2ULL * world * 4 + 2ULL * world * 8 + 64;
    char *w = (char *)workspace(4, need);
    if (!w) return ZKGPU_ERR_OOM;
    uint32_t *tslots = (uint32_t *)w, *fslots = tslots + m, *fcnt = fslots + m, *cnt = fcnt + m;
    uint64_t *base = (uint64_t *)(((uintptr_t)(cnt + 2 * world) + 7) & ~(uintptr_t)7);
    const uint32_t B = 256;
    prof_begin(s);
    if (check_hip(hipMemsetAsync(tslots, 0xFF, 2 * m * 4, s), "h1h2 memset") ||
        check_hip(hipMemsetAsync(fcnt, 0, m * 4 + 2ULL * world * 4, s), "h1h2 memset"))
        return ZKGPU_ERR_HIP;
    if (dim == 1) {
        hipLaunchKernelGGL(k_h12_insert<1>, dim3(nblk2(n, B)), dim3(B), 0, s, tslots, m - 1, t, t_ld, n);
        hipLaunchKernelGGL(k_h12s_insert_f<1>, dim3(nblk2(n, B)), dim3(B), 0, s, fslots, fcnt, m - 1, f, f_ld, n);
        hipLaunchKernelGGL(k_h12s_bucket<1>, dim3(nblk2(2 * m, B)), dim3(B), 0, s, recs, tslots, fslots, fcnt, m, t,
                           t_ld, f, f_ld, row0, world, cnt, (const uint64_t *)base, 0);
    } else {
        hipLaunchKernelGGL(k_h12_insert<3>, dim3(nblk2(n, B)), dim3(B), 0, s, tslots, m - 1, t, t_ld, n);
        hipLaunchKernelGGL(k_h12s_insert_f<3>, dim3(nblk2(n, B)), dim3(B), 0, s, fslots, fcnt, m - 1, f, f_ld, n);
        hipLaunchKernelGGL(k_h12s_bucket<3>, dim3(nblk2(2 * m, B)), dim3(B), 0, s, recs, tslots, fslots, fcnt, m, t,
                           t_ld, f, f_ld, row0, world, cnt, (const uint64_t *)base, 0);
    }
    std::vector<uint32_t> c(2 * world);
    if (check_hip(hipMemcpyAsync(c.data(), cnt, 2ULL * world * 4, hipMemcpyDeviceToHost, s), "D2H") ||
        check_hip(hipStreamSynchronize(s), "h1h2 sync"))
        return ZKGPU_ERR_HIP;
    // buckets in owner order, t records first in each
    std::vector<uint64_t> b(2 * world);
    uint64_t off = 0;
    for (uint32_t o = 0; o < world; o++) {
        n_t[o] = c[2 * o];
        n_f[o] = c[2 * o + 1];
        b[2 * o] = off;
        b[2 * o + 1] = off + c[2 * o];
        off += (uint64_t)c[2 * o] + c[2 * o + 1];
    }
    if (off > cap)
        return set_error(ZKGPU_ERR_ARG, "h1h2 (sharded): %llu records exceed the %llu-record buffer",
                         (unsigned long long)off, (unsigned long long)cap);
    if (check_hip(hipMemcpyAsync(base, b.data(), 2ULL * world * 8, hipMemcpyHostToDevice, s), "H2D") ||
        check_hip(hipMemsetAsync(cnt, 0, 2ULL * world * 4, s), "h1h2 memset"))
        return ZKGPU_ERR_HIP;
    if (dim == 1)
        hipLaunchKernelGGL(k_h12s_bucket<1>, dim3(nblk2(2 * m, B)), dim3(B), 0, s, recs, tslots, fslots, fcnt, m, t,
                           t_ld, f, f_ld, row0, world, cnt, (const uint64_t *)base, 1);
    else
        hipLaunchKernelGGL(k_h12s_bucket<3>, dim3(nblk2(2 * m, B)), dim3(B), 0, s, recs, tslots, fslots, fcnt, m, t,
                           t_ld, f, f_ld, row0, world, cnt, (const uint64_t *)base, 1);
    if (check_hip(hipStreamSynchronize(s), "h1h2 sync")) return ZKGPU_ERR_HIP;  // b dies here
    prof_end("k_h1h2_route", (double)dim * 8.0 * 2.0 * n, s);
    return check_launch("h1h2 route");
}

int h1h2_shard_owner(uint64_t *ret, const uint64_t *recs, uint64_t nrec, uint32_t dim, uint64_t *miss_row,
                     hipStream_t s)
{
    const uint64_t m = h12s_table_size(nrec);
    const size_t need = m * 8 + nrec * 8 + 16;
    char *w = (char *)workspace(4, need);
    if (!w) return ZKGPU_ERR_OOM;
    unsigned long long *slots = (unsigned long long *)w, *sum = slots + m, *miss = sum + nrec;
    const uint32_t B = 256;
    prof_begin(s);
    if (check_hip(hipMemsetAsync(slots, 0, (m + nrec) * 8, s), "h1h2 memset") ||
        check_hip(hipMemsetAsync(miss, 0xFF, 8, s), "h1h2 memset"))
        return ZKGPU_ERR_HIP;
    if (nrec) {
        if (dim == 1) {
            hipLaunchKernelGGL(k_h12s_own_insert<1>, dim3(nblk2(nrec, B)), dim3(B), 0, s, slots, m - 1, recs, nrec);
            hipLaunchKernelGGL(k_h12s_own_probe<1>, dim3(nblk2(nrec, B)), dim3(B), 0, s, slots, m - 1, recs, nrec, sum,
                               miss);
            hipLaunchKernelGGL(k_h12s_own_ret<1>, dim3(nblk2(nrec, B)), dim3(B), 0, s, ret, slots, m - 1, recs, nrec,
                               sum);
        } else {
            hipLaunchKernelGGL(k_h12s_own_insert<3>, dim3(nblk2(nrec, B)), dim3(B), 0, s, slots, m - 1, recs, nrec);
            hipLaunchKernelGGL(k_h12s_own_probe<3>, dim3(nblk2(nrec, B)), dim3(B), 0, s, slots, m - 1, recs, nrec, sum,
                               miss);
            hipLaunchKernelGGL(k_h12s_own_ret<3>, dim3(nblk2(nrec, B)), dim3(B), 0, s, ret, slots, m - 1, recs, nrec,
                               sum);
        }
    }
    unsigned long long mh = 0;
    if (check_hip(hipMemcpyAsync(&mh, miss, 8, hipMemcpyDeviceToHost, s), "D2H") ||
        check_hip(hipStreamSynchronize(s), "h1h2 sync"))
        return ZKGPU_ERR_HIP;
    *miss_row = mh;
    prof_end("k_h1h2_owner", 40.0 * (double)nrec, s);
    return check_launch("h1h2 owner");
}

int h1h2_shard_counts(uint32_t *start, uint32_t *cnt, uint64_t *total, const uint64_t *sent, const uint64_t *ret,
                      uint64_t nsent, uint64_t n, uint64_t row0, hipStream_t s)
{
    size_t scan_bytes = 0;
    if (rocprim::exclusive_scan(nullptr, scan_bytes, cnt, start, 0u, (size_t)n, rocprim::plus<uint32_t>(), s) !=
        hipSuccess)
        return set_error(ZKGPU_ERR_HIP, "h1h2: rocprim temp-size query failed");
    void *tmp = workspace(5, scan_bytes);
    if (!tmp) return ZKGPU_ERR_OOM;
    const uint32_t B = 256;
    hipLaunchKernelGGL(k_h12_fill1, dim3(nblk2(n, B)), dim3(B), 0, s, cnt, n);
    if (nsent) hipLaunchKernelGGL(k_h12s_apply, dim3(nblk2(nsent, B)), dim3(B), 0, s, cnt, sent, ret, nsent, row0);
    size_t tb = scan_bytes;
    if (rocprim::exclusive_scan(tmp, tb, cnt, start, 0u, (size_t)n, rocprim::plus<uint32_t>(), s) != hipSuccess)
        return set_error(ZKGPU_ERR_HIP, "h1h2: scan failed");
    uint32_t last[2] = {0, 0};
    if (check_hip(hipMemcpyAsync(&last[0], start + n - 1, 4, hipMemcpyDeviceToHost, s), "D2H") ||
        check_hip(hipMemcpyAsync(&last[1], cnt + n - 1, 4, hipMemcpyDeviceToHost, s), "D2H") ||
        check_hip(hipStreamSynchronize(s), "h1h2 sync"))
        return ZKGPU_ERR_HIP;
    *total = (uint64_t)last[0] + last[1];
    return check_launch("h1h2 counts");
}

int h1h2_shard_deal(uint64_t *seg, uint64_t seg_ld, const uint64_t *t, uint64_t t_ld, const uint32_t *start,
                    const uint32_t *cnt, uint64_t n, uint32_t dim, hipStream_t s)
{
    const uint32_t B = 256;
    if (dim == 1)
        hipLaunchKernelGGL(k_h12s_deal<1>, dim3(nblk2(n, B)), dim3(B), 0, s, seg, seg_ld, t, t_ld, start, cnt, n);
    else
        hipLaunchKernelGGL(k_h12s_deal<3>, dim3(nblk2(n, B)), dim3(B), 0, s, seg, seg_ld, t, t_ld, start, cnt, n);
    return check_launch("h1h2 deal");
}

int h1h2_shard_place(uint64_t *h1, uint64_t h1_ld, uint64_t *h2, uint64_t h2_ld, const uint64_t *buf, uint64_t buf_ld,
                     uint64_t pos0, uint64_t len, uint64_t row0, uint32_t dim, hipStream_t s)
{
    if (!len) return 0;
    const uint32_t B = 256;
    if (dim == 1)
        hipLaunchKernelGGL(k_h12s_place<1>, dim3(nblk2(len, B)), dim3(B), 0, s, h1, h1_ld, h2, h2_ld, buf, buf_ld, pos0,
                           len, row0);
    else
        hipLaunchKernelGGL(k_h12s_place<3>, dim3(nblk2(len, B)), dim3(B), 0, s, h1, h1_ld, h2, h2_ld, buf, buf_ld, pos0,
                           len, row0);
    return check_launch("h1h2 place");
}

// ---------------------------------------------------------------- multiset difference
// The distinct values of two n-row columns a and b whose multiplicities
// differ (the prover's calculateZ diagnosis: a permutation check that does not
// close; include/zkgpu.h zkgpu_multiset_diff_dev).  One open-addressing table
// of rows, keyed like the plookup's, holds the up to 2n distinct values of
// both columns at load <= 0.5 (2^k >= 4n slots).  Row i of a has index i, row
// i of b index n + i; per slot:
//   slot    the SMALLEST index with the slot's key (atomicMin): below n it is
//           the value's first row in a
//   firstb  the value's first row in b (atomicMin)
//   cnta / cntb  its rows in a / in b (atomicAdd)
// Which thread claims an empty slot decides only WHERE a key lives, never
// what the slot ends up holding: minima and sums do not depend on the order.
// k_ms_flag then marks, for every slot with cnta != cntb, the value's first
// row in a flag column per side, the nonzero-rows reduction (stark.hip,
// independent of the launch geometry) lists the lowest max_vals of each, and
// k_ms_emit looks every listed row's slot up again for its two counts.
constexpr uint32_t MS_MAX_VALS = 4096;  // = NZ_MAX_ROWS (the lists come from k_nz_emit)

static uint64_t ms_table_size(uint64_t n)
{
    if (!n) return 0;
    uint64_t m = 1;
    while (m < 4 * n) m <<= 1;
    return m;
}

struct MsTable {
    uint32_t *slot, *firstb, *cnta, *cntb;
    uint64_t mask;
    const uint64_t *a, *b;
    uint64_t a_ld, b_ld, n;
};

// does the row with index g (a: g, b: n + g) hold key?
template <int DIM>
__device__ __forceinline__ bool ms_eq(const MsTable &T, uint32_t g, const uint64_t key[DIM])
{
    return g < T.n ? h12_eq<DIM>(T.a, T.a_ld, g, key) : h12_eq<DIM>(T.b, T.b_ld, g - (uint32_t)T.n, key);
}

template <int DIM>
__global__ void __launch_bounds__(256) k_ms_insert(MsTable T)
{
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = g < 2 * T.n;
    const bool side = g >= T.n;
    const uint64_t i = side ? g - T.n : g;
    uint32_t *ctr = nullptr;
    if (live) {
        uint64_t key[DIM];
        h12_key<DIM>(key, side ? T.b : T.a, side ? T.b_ld : T.a_ld, i);
        uint64_t h = h12_hash<DIM>(key) & T.mask;
        // bounded by the table size; 2n indices in >= 4n slots: a slot is always found
        for (uint64_t probe = 0; probe <= T.mask; probe++, h = (h + 1) & T.mask) {
            uint32_t cur = T.slot[h];
            if (cur == H12_EMPTY) {
                cur = atomicCAS(&T.slot[h], H12_EMPTY, (uint32_t)g);
                if (cur == H12_EMPTY) cur = (uint32_t)g;
            }
            if (cur == (uint32_t)g || ms_eq<DIM>(T, cur, key)) {  // every index a slot ever holds has its key
                if (cur > (uint32_t)g) atomicMin(&T.slot[h], (uint32_t)g);  // (a slot only ever decreases)
                if (side && T.firstb[h] > (uint32_t)i) atomicMin(&T.firstb[h], (uint32_t)i);
                ctr = side ? &T.cntb[h] : &T.cnta[h];
                break;
            }
        }
    }
    // one add per wave for the lanes that share the first lane's counter (a
    // permutation's default value sits on most rows), one per lane otherwise
    const uint64_t todo = __ballot(ctr != nullptr);
    if (!todo) return;
    const int lead = __ffsll((unsigned long long)todo) - 1;
    const uint64_t p = (uint64_t)ctr;
    const uint64_t lp = ((uint64_t)(uint32_t)__shfl((int)(p >> 32), lead) << 32) | (uint32_t)__shfl((int)p, lead);
    const uint64_t same = __ballot(ctr != nullptr && p == lp);
    if (!ctr) return;
    if (p != lp)
        atomicAdd(ctr, 1u);
    else if ((int)(threadIdx.x & 63) == lead)
        atomicAdd(ctr, (uint32_t)__popcll(same));
}

// slot k with unequal counts -> flag the value's first row on each side it occurs on
__global__ void __launch_bounds__(256) k_ms_flag(uint64_t *flaga, uint64_t *flagb, MsTable T)
{
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k > T.mask) return;
    const uint32_t g = T.slot[k];
    if (g == H12_EMPTY || T.cnta[k] == T.cntb[k]) return;
    if (g < T.n) flaga[g] = 1;
    const uint32_t fb = T.firstb[k];
    if (fb != H12_EMPTY) flagb[fb] = 1;
}

// block y (0: a, 1: b) of out from the side's row list {count, rows ...}
template <int DIM>
__global__ void __launch_bounds__(256) k_ms_emit(uint64_t *out, const uint64_t *lista, const uint64_t *listb,
                                                 uint32_t max_vals, MsTable T)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    const bool side = blockIdx.y;
    const uint64_t *list = side ? listb : lista;
    uint64_t *o = out + (side ? 1 + 3ULL * max_vals : 0);
    if (k == 0) o[0] = list[0];
    if (k >= max_vals) return;
    const uint64_t row = list[1 + k];
    uint64_t ca = 0, cb = 0;
    if (row < T.n) {
        uint64_t key[DIM];
        h12_key<DIM>(key, side ? T.b : T.a, side ? T.b_ld : T.a_ld, row);
        uint64_t h = h12_hash<DIM>(key) & T.mask;
        for (uint64_t probe = 0; probe <= T.mask; probe++, h = (h + 1) & T.mask) {
            const uint32_t cur = T.slot[h];
            if (cur == H12_EMPTY) break;
            if (ms_eq<DIM>(T, cur, key)) {
                ca = T.cnta[h];
                cb = T.cntb[h];
                break;
            }
        }
    }
    o[1 + 3ULL * k] = row;
    o[2 + 3ULL * k] = ca;
    o[3 + 3ULL * k] = cb;
}

// the layout of the workspace (include/zkgpu.h states the sum)
struct MsLayout {
    uint64_t m, table, flags, counts, lists, total;
};
static MsLayout ms_layout(uint64_t n)
{
    MsLayout L;
    L.m = ms_table_size(n);
    L.table = 0;                                                      // slot, firstb, cnta, cntb: 4 x m u32
    L.flags = L.table + 16 * L.m;                                     // 2 flag columns of n u64
    L.counts = L.flags + 16 * n;                                      // the nonzero-rows block counts
    L.lists = L.counts + 8 * (((uint64_t)nonzero_rows_blocks(n) + 1) / 2);  // 2 lists of 1 + MS_MAX_VALS u64
    L.total = L.lists + 2 * 8 * (1 + (uint64_t)MS_MAX_VALS);
    return L;
}

uint64_t multiset_diff_workspace_bytes(uint64_t n) { return ms_layout(n).total; }

int multiset_diff(uint64_t *out, const uint64_t *a, uint64_t a_ld, const uint64_t *b, uint64_t b_ld, uint64_t n,
                  uint32_t dim, uint32_t max_vals, hipStream_t s)
{
    const MsLayout L = ms_layout(n);
    char *w = (char *)workspace(4, L.total);
    if (!w) return ZKGPU_ERR_OOM;
    MsTable T;
    T.slot = (uint32_t *)(w + L.table);
    T.firstb = T.slot + L.m;
    T.cnta = T.firstb + L.m;
    T.cntb = T.cnta + L.m;
    T.mask = L.m - 1;
    T.a = a, T.b = b, T.a_ld = a_ld, T.b_ld = b_ld, T.n = n;
    uint64_t *flaga = (uint64_t *)(w + L.flags), *flagb = flaga + n;
    uint32_t *counts = (uint32_t *)(w + L.counts);
    uint64_t *lista = (uint64_t *)(w + L.lists), *listb = lista + 1 + MS_MAX_VALS;
    const uint32_t B = 256;
    if (n) {
        prof_begin(s);
        // slot and firstb empty, the counts and the flags zero
        if (check_hip(hipMemsetAsync(T.slot, 0xFF, 8 * L.m, s), "multiset_diff memset") ||
            check_hip(hipMemsetAsync(T.cnta, 0, 8 * L.m + 16 * n, s), "multiset_diff memset"))
            return ZKGPU_ERR_HIP;
        if (dim == 1)
            hipLaunchKernelGGL(k_ms_insert<1>, dim3(nblk2(2 * n, B)), dim3(B), 0, s, T);
        else
            hipLaunchKernelGGL(k_ms_insert<3>, dim3(nblk2(2 * n, B)), dim3(B), 0, s, T);
        prof_end("k_multiset_insert", (double)dim * 8.0 * 2.0 * n, s);
        prof_begin(s);
        hipLaunchKernelGGL(k_ms_flag, dim3(nblk2(L.m, B)), dim3(B), 0, s, flaga, flagb, T);
        prof_end("k_multiset_flag", 16.0 * (double)L.m, s);
        if (check_launch("multiset_diff")) return ZKGPU_ERR_HIP;
    }
    int rc;
    if ((rc = nonzero_rows(lista, counts, flaga, n, 1, n, max_vals, s)) ||
        (rc = nonzero_rows(listb, counts, flagb, n, 1, n, max_vals, s)))
        return rc;
    prof_begin(s);
    const dim3 grid(nblk2(max_vals ? max_vals : 1, B), 2);
    if (dim == 1)
        hipLaunchKernelGGL(k_ms_emit<1>, grid, dim3(B), 0, s, out, lista, listb, max_vals, T);
    else
        hipLaunchKernelGGL(k_ms_emit<3>, grid, dim3(B), 0, s, out, lista, listb, max_vals, T);
    prof_end("k_multiset_emit", 2.0 * 8.0 * (1 + 3.0 * max_vals), s);
    return check_launch("multiset_diff");
}

// ---------------------------------------------------------------- lookup misses
// The f values of a plookup that no row of its table t holds (the prover's
// trace audit; include/zkgpu.h zkgpu_lookup_misses_dev).  The table is the
// multiset table above over a = f and b = t (k_ms_insert as it stands): a value
// misses iff its slot ends with cntb = 0, its slot is then its first row in f
// and cnta its rows there.  k_lookup_flag walks the slots once: it flags the
// first row of every missing value and adds up their cnta -- the rows that
// miss -- per thread, then per wave and workgroup, so that one atomic per
// workgroup reaches the global sum (a sum of integers: the grid does not
// change it).  The nonzero-rows reduction lists the lowest max_vals flagged
// rows and counts all of them (the distinct values); k_lookup_emit looks each
// listed row's count up again.
constexpr uint32_t LM_FLAG_BLOCKS = 1024;  // grid-stride cap of k_lookup_flag

__global__ void __launch_bounds__(256) k_lookup_flag(uint64_t *flag, unsigned long long *n_rows, MsTable T)
{
    __shared__ uint32_t part[4];
    // a thread's sum is part of the sum of all cnta = n <= 2^28: u32 holds it
    uint32_t sum = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k <= T.mask; k += stride) {
        const uint32_t g = T.slot[k];
        if (g == H12_EMPTY || g >= T.n || T.cntb[k]) continue;  // empty, a value of t only, or a value t holds
        flag[g] = 1;
        sum += T.cnta[k];
    }
#pragma unroll
    for (int off = 32; off; off >>= 1) sum += (uint32_t)__shfl_down((int)sum, off);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t tot = part[0] + part[1] + part[2] + part[3];
        if (tot) atomicAdd(n_rows, (unsigned long long)tot);
    }
}

// out = {rows that miss, distinct values, then per listed row {row, its value's rows in f}}
template <int DIM>
__global__ void __launch_bounds__(256) k_lookup_emit(uint64_t *out, const uint64_t *list,
                                                     const unsigned long long *n_rows, uint32_t max_vals, MsTable T)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k == 0) {
        out[0] = *n_rows;
        out[1] = list[0];
    }
    if (k >= max_vals) return;
    const uint64_t row = list[1 + k];
    uint64_t cnt = 0;
    if (row < T.n) {
        uint64_t key[DIM];
        h12_key<DIM>(key, T.a, T.a_ld, row);
        uint64_t h = h12_hash<DIM>(key) & T.mask;
        for (uint64_t probe = 0; probe <= T.mask; probe++, h = (h + 1) & T.mask) {
            const uint32_t cur = T.slot[h];
            if (cur == H12_EMPTY) break;
            if (ms_eq<DIM>(T, cur, key)) {
                cnt = T.cnta[h];
                break;
            }
        }
    }
    out[2 + 2ULL * k] = row;  // (the reduction pads its list with UINT64_MAX)
    out[3 + 2ULL * k] = cnt;
}

// the layout of the workspace (include/zkgpu.h states the sum): the multiset
// table, ONE flag column and list, and the word the missing rows add up in
struct LmLayout {
    uint64_t m, table, flags, counts, list, sum, total;
};
static LmLayout lm_layout(uint64_t n)
{
    LmLayout L;
    L.m = ms_table_size(n);
    L.table = 0;
    L.flags = L.table + 16 * L.m;
    L.counts = L.flags + 8 * n;
    L.list = L.counts + 8 * (((uint64_t)nonzero_rows_blocks(n) + 1) / 2);
    L.sum = L.list + 8 * (1 + (uint64_t)MS_MAX_VALS);
    L.total = L.sum + 8;
    return L;
}

uint64_t lookup_misses_workspace_bytes(uint64_t n) { return lm_layout(n).total; }

int lookup_misses(uint64_t *out, const uint64_t *f, uint64_t f_ld, const uint64_t *t, uint64_t t_ld, uint64_t n,
                  uint32_t dim, uint32_t max_vals, hipStream_t s)
{
    const LmLayout L = lm_layout(n);
    char *w = (char *)workspace(4, L.total);
    if (!w) return ZKGPU_ERR_OOM;
    MsTable T;
    T.slot = (uint32_t *)(w + L.table);
    T.firstb = T.slot + L.m;
    T.cnta = T.firstb + L.m;
    T.cntb = T.cnta + L.m;
    T.mask = L.m - 1;
    T.a = f, T.b = t, T.a_ld = f_ld, T.b_ld = t_ld, T.n = n;
    uint64_t *flag = (uint64_t *)(w + L.flags);
    uint32_t *counts = (uint32_t *)(w + L.counts);
    uint64_t *list = (uint64_t *)(w + L.list);
    unsigned long long *sum = (unsigned long long *)(w + L.sum);
    const uint32_t B = 256;
    if (check_hip(hipMemsetAsync(sum, 0, 8, s), "lookup_misses memset")) return ZKGPU_ERR_HIP;
    if (n) {
        prof_begin(s);
        // slot and firstb empty, the counts and the flags zero
        if (check_hip(hipMemsetAsync(T.slot, 0xFF, 8 * L.m, s), "lookup_misses memset") ||
            check_hip(hipMemsetAsync(T.cnta, 0, 8 * L.m + 8 * n, s), "lookup_misses memset"))
            return ZKGPU_ERR_HIP;
        if (dim == 1)
            hipLaunchKernelGGL(k_ms_insert<1>, dim3(nblk2(2 * n, B)), dim3(B), 0, s, T);
        else
            hipLaunchKernelGGL(k_ms_insert<3>, dim3(nblk2(2 * n, B)), dim3(B), 0, s, T);
        prof_end("k_multiset_insert", (double)dim * 8.0 * 2.0 * n, s);
        prof_begin(s);
        hipLaunchKernelGGL(k_lookup_flag, dim3(std::min(nblk2(L.m, B), LM_FLAG_BLOCKS)), dim3(B), 0, s, flag, sum, T);
        prof_end("k_lookup_flag", 12.0 * (double)L.m, s);
        if (check_launch("lookup_misses")) return ZKGPU_ERR_HIP;
    }
    int rc;
    if ((rc = nonzero_rows(list, counts, flag, n, 1, n, max_vals, s))) return rc;
    prof_begin(s);
    if (dim == 1)
        hipLaunchKernelGGL(k_lookup_emit<1>, dim3(nblk2(max_vals ? max_vals : 1, B)), dim3(B), 0, s, out, list, sum,
                           max_vals, T);
    else
        hipLaunchKernelGGL(k_lookup_emit<3>, dim3(nblk2(max_vals ? max_vals : 1, B)), dim3(B), 0, s, out, list, sum,
                           max_vals, T);
    prof_end("k_lookup_emit", 8.0 * (2 + 2.0 * max_vals), s);
    return check_launch("lookup_misses");
}

}  // namespace zk

// the C-ABI of the lookup misses (include/zkgpu.h), beside its kernels
extern "C" uint64_t zkgpu_lookup_misses_workspace_bytes(uint64_t n) { return zk::lookup_misses_workspace_bytes(n); }

extern "C" int zkgpu_lookup_misses_dev(uint64_t *out, const uint64_t *f, uint64_t f_ld, const uint64_t *t,
                                       uint64_t t_ld, uint64_t n, uint32_t dim, uint32_t max_vals)
{
    if (!zk::ctx().ready) return zk::set_error(ZKGPU_ERR_INIT, "zkgpu_init() not called");
    if (!out || (n && (!f || !t))) return zk::set_error(ZKGPU_ERR_ARG, "lookup_misses: null pointer");
    if (dim != 1 && dim != 3) return zk::set_error(ZKGPU_ERR_ARG, "lookup_misses: dim must be 1 or 3");
    if (max_vals > zk::MS_MAX_VALS)
        return zk::set_error(ZKGPU_ERR_ARG, "lookup_misses: max_vals %u > %u", max_vals, zk::MS_MAX_VALS);
    if (n > (1ULL << 28)) return zk::set_error(ZKGPU_ERR_ARG, "lookup_misses: more than 2^28 rows");
    if (f_ld < n || t_ld < n) return zk::set_error(ZKGPU_ERR_ARG, "lookup_misses: ld < n");
    return zk::lookup_misses(out, f, f_ld, t, t_ld, n, dim, max_vals, zk::ctx().stream);
}

// the C-ABI of the multiset difference (include/zkgpu.h), beside its kernels
extern "C" uint64_t zkgpu_multiset_diff_workspace_bytes(uint64_t n) { return zk::multiset_diff_workspace_bytes(n); }

extern "C" int zkgpu_multiset_diff_dev(uint64_t *out, const uint64_t *a, uint64_t a_ld, const uint64_t *b,
                                       uint64_t b_ld, uint64_t n, uint32_t dim, uint32_t max_vals)
{
    if (!zk::ctx().ready) return zk::set_error(ZKGPU_ERR_INIT, "zkgpu_init() not called");
    if (!out || (n && (!a || !b))) return zk::set_error(ZKGPU_ERR_ARG, "multiset_diff: null pointer");
    if (dim != 1 && dim != 3) return zk::set_error(ZKGPU_ERR_ARG, "multiset_diff: dim must be 1 or 3");
    if (max_vals > zk::MS_MAX_VALS)
        return zk::set_error(ZKGPU_ERR_ARG, "multiset_diff: max_vals %u > %u", max_vals, zk::MS_MAX_VALS);
    if (n > (1ULL << 28)) return zk::set_error(ZKGPU_ERR_ARG, "multiset_diff: more than 2^28 rows");
    if (a_ld < n || b_ld < n) return zk::set_error(ZKGPU_ERR_ARG, "multiset_diff: ld < n");
    return zk::multiset_diff(out, a, a_ld, b, b_ld, n, dim, max_vals, zk::ctx().stream);
}
