// Circom .exec hand-off on the GPU (zkgpu_exec_*, include/zkgpu.h): the
// reference's Circom*::getCommitedPols loop (main.recursive1.cpp:343-394) from
// a witness of sizeWitness words to the committed columns, column-major on
// the device.  The plan (levels, launch segments, transposed sMap) is made on
// the host once per circuit (csrc/exec_plan.cpp); a commit uploads the witness
// and runs one kernel per segment, then the gather.
//
// tmp holds lazy words (any u64 is an element): the witness as it came, the
// adds' results canonical.  The gather canonicalises what it stores.
#include <initializer_list>
#include <new>
#include <vector>

#include "exec_plan.hpp"
#include "gl_device.hpp"
#include "zkgpu_internal.hpp"

namespace zk {

// one level over the grid: adds [first, first + count) of the sorted tables
__global__ void __launch_bounds__(256) k_exec_adds_level(uint64_t *tmp, const uint32_t *a, const uint32_t *b,
                                                         const uint64_t *c, const uint64_t *d, const uint32_t *dst,
                                                         uint32_t first, uint32_t count)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= count) return;
    const uint32_t k = first + t;
    tmp[dst[k]] = gl_canon(gl_add(gl_mul(tmp[a[k]], c[k]), gl_mul(tmp[b[k]], d[k])));
}

// one workgroup, levels [l0, l0 + nl) of at most blockDim.x adds each:
// level_end[l] is the sorted position one past level l's last add.  The
// barrier orders a level's stores before the next level's loads (the
// workgroup's waves share the CU's vector cache).
__global__ void __launch_bounds__(EXEC_TAIL_MAX) k_exec_adds_tail(uint64_t *tmp, const uint32_t *a, const uint32_t *b,
                                                                  const uint64_t *c, const uint64_t *d,
                                                                  const uint32_t *dst, const uint32_t *level_end,
                                                                  uint32_t first, uint32_t l0, uint32_t nl)
{
    // A level's records do not depend on the level before it, only its tmp
    // operands do: the next level's records are loaded while this level's
    // operands are in flight, so a level costs one dependent round trip, not two.
    uint32_t ra = 0, rb = 0, rdst = 0;
    uint64_t rc = 0, rd = 0;
    uint32_t end = level_end[l0];
    bool act = first + threadIdx.x < end;
    if (act) {
        const uint32_t k = first + threadIdx.x;
        ra = a[k], rb = b[k], rc = c[k], rd = d[k], rdst = dst[k];
    }
    for (uint32_t l = l0; l < l0 + nl; l++) {
        const bool more = l + 1 < l0 + nl;
        const uint32_t nend = more ? level_end[l + 1] : end;
        const uint32_t nk = end + threadIdx.x;
        const bool nact = more && nk < nend;
        uint64_t x = 0, y = 0;
        if (act) x = tmp[ra], y = tmp[rb];
        uint32_t na = 0, nb = 0, ndst = 0;
        uint64_t nc = 0, nd = 0;
        if (nact) na = a[nk], nb = b[nk], nc = c[nk], nd = d[nk], ndst = dst[nk];
        if (act) tmp[rdst] = gl_canon(gl_add(gl_mul(x, rc), gl_mul(y, rd)));
        ra = na, rb = nb, rc = nc, rd = nd, rdst = ndst;
        act = nact;
        end = nend;
        __syncthreads();
    }
}

// cols[j * ld + i] for i < n, j = blockIdx.y: the sMap cell's slot, 0 for an
// empty cell (index 0) and for the rows past nSMap
__global__ void __launch_bounds__(256) k_exec_gather(uint64_t *cols, uint64_t ld, uint64_t n, const uint64_t *tmp,
                                                     const uint32_t *smap_t, uint64_t n_smap)
{
    const uint32_t j = blockIdx.y;
    uint64_t *col = cols + (uint64_t)j * ld;
    const uint32_t *sm = smap_t + (uint64_t)j * n_smap;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u) {
        const uint32_t idx = i < n_smap ? sm[i] : 0u;
        col[i] = idx ? gl_canon(tmp[idx]) : 0ULL;
    }
}

namespace {

struct Exec {
    ExecPlan plan;
    char *blob = nullptr;  // one device allocation: the tables below, then tmp
    uint64_t bytes = 0;
    uint32_t *a = nullptr, *b = nullptr, *dst = nullptr, *level_end = nullptr, *smap_t = nullptr;
    uint64_t *c = nullptr, *d = nullptr, *tmp = nullptr;
};

uint64_t up256(uint64_t x) { return (x + 255) & ~255ULL; }

uint32_t g_tail_width = 0;  // zkgpu_exec_set_tail_width (0: EXEC_TAIL_MAX)

}  // namespace

}  // namespace zk

using namespace zk;

extern "C" int zkgpu_exec_create(void **exec, const uint64_t *image, uint64_t image_words, uint64_t size_witness,
                                 uint32_t n_cols)
{
    if (!exec) return set_error(ZKGPU_ERR_ARG, "exec_create: null pointer");
    *exec = nullptr;
    if (!ctx().ready) return set_error(ZKGPU_ERR_INIT, "zkgpu_init() not called");
    Exec *e = new (std::nothrow) Exec();
    if (!e) return set_error(ZKGPU_ERR_OOM, "exec_create: out of host memory");
    int rc = exec_plan_build(e->plan, image, image_words, size_witness, n_cols, g_tail_width);
    if (rc) {
        delete e;
        return rc;
    }
    const ExecPlan &P = e->plan;
    // layout: u64 tables first, then the u32 ones, each 256-byte aligned
    const uint64_t na = P.n_adds, o_c = 0, o_d = o_c + up256(na * 8), o_tmp = o_d + up256(na * 8),
                   o_a = o_tmp + up256((P.size_witness + na) * 8), o_b = o_a + up256(na * 4), o_dst = o_b + up256(na * 4),
                   o_le = o_dst + up256(na * 4), o_sm = o_le + up256((uint64_t)P.n_levels * 4);
    e->bytes = o_sm + up256((uint64_t)P.smap_t.size() * 4);
    if (hipMalloc((void **)&e->blob, e->bytes) != hipSuccess) {
        const uint64_t bytes = e->bytes;
        delete e;
        return set_error(ZKGPU_ERR_OOM, "exec_create: hipMalloc(%llu) of the plan's tables and tmp failed",
                         (unsigned long long)bytes);
    }
    e->c = (uint64_t *)(e->blob + o_c);
    e->d = (uint64_t *)(e->blob + o_d);
    e->tmp = (uint64_t *)(e->blob + o_tmp);
    e->a = (uint32_t *)(e->blob + o_a);
    e->b = (uint32_t *)(e->blob + o_b);
    e->dst = (uint32_t *)(e->blob + o_dst);
    e->level_end = (uint32_t *)(e->blob + o_le);
    e->smap_t = (uint32_t *)(e->blob + o_sm);
    hipStream_t s = ctx().stream;
    auto up = [&](void *dp, const void *hp, uint64_t bytes) {
        return bytes ? check_hip(hipMemcpyAsync(dp, hp, bytes, hipMemcpyHostToDevice, s), "exec_create H2D") : 0;
    };
    if ((rc = up(e->c, P.c.data(), na * 8)) || (rc = up(e->d, P.d.data(), na * 8)) || (rc = up(e->a, P.a.data(), na * 4)) ||
        (rc = up(e->b, P.b.data(), na * 4)) || (rc = up(e->dst, P.dst.data(), na * 4)) ||
        (rc = up(e->level_end, P.level_end.data(), (uint64_t)P.n_levels * 4)) ||
        (rc = up(e->smap_t, P.smap_t.data(), (uint64_t)P.smap_t.size() * 4)) ||
        (rc = check_hip(hipStreamSynchronize(s), "exec_create sync"))) {
        (void)hipFree(e->blob);
        delete e;
        return rc;
    }
    // the host copies of the tables are on the device now; the segments and the counts stay
    Exec *keep = e;
    for (auto *v : {&keep->plan.a, &keep->plan.b, &keep->plan.dst, &keep->plan.smap_t, &keep->plan.level})
        std::vector<uint32_t>().swap(*v);
    std::vector<uint64_t>().swap(keep->plan.c);
    std::vector<uint64_t>().swap(keep->plan.d);
    *exec = e;
    return 0;
}

extern "C" void zkgpu_exec_set_tail_width(uint32_t max_adds) { g_tail_width = max_adds; }

extern "C" int zkgpu_exec_info(void *exec, uint64_t *n_adds, uint64_t *n_smap, uint32_t *n_levels,
                               uint32_t *n_launches, uint64_t *device_bytes)
{
    if (!exec) return set_error(ZKGPU_ERR_ARG, "exec_info: null handle");
    const Exec *e = (const Exec *)exec;
    if (n_adds) *n_adds = e->plan.n_adds;
    if (n_smap) *n_smap = e->plan.n_smap;
    if (n_levels) *n_levels = e->plan.n_levels;
    if (n_launches) *n_launches = (uint32_t)e->plan.segs.size() + 1;  // the segments and the gather
    if (device_bytes) *device_bytes = e->bytes;
    return 0;
}

extern "C" int zkgpu_exec_commit_dev(void *exec, const uint64_t *witness, uint64_t *cols, uint64_t ld, uint64_t n)
{
    if (!ctx().ready) return set_error(ZKGPU_ERR_INIT, "zkgpu_init() not called");
    if (!exec || !witness) return set_error(ZKGPU_ERR_ARG, "exec_commit: null pointer");
    Exec *e = (Exec *)exec;
    const ExecPlan &P = e->plan;
    if (n < P.n_smap)
        return set_error(ZKGPU_ERR_ARG, "exec_commit: n = %llu rows, fewer than the sMap's %llu", (unsigned long long)n,
                         (unsigned long long)P.n_smap);
    if (n > ld)
        return set_error(ZKGPU_ERR_ARG, "exec_commit: n = %llu above ld = %llu", (unsigned long long)n,
                         (unsigned long long)ld);
    if (n && !cols) return set_error(ZKGPU_ERR_ARG, "exec_commit: null pointer");
    hipStream_t s = ctx().stream;
    // the caller's buffer is free again when this returns: the copy is waited for, the kernels are not
    int rc = check_hip(hipMemcpyAsync(e->tmp, witness, P.size_witness * 8, hipMemcpyHostToDevice, s), "exec_commit H2D");
    if (!rc) rc = check_hip(hipStreamSynchronize(s), "exec_commit H2D sync");
    if (rc) return rc;
    for (const ExecSegment &g : P.segs) {
        prof_begin(s);
        if (g.grid) {
            hipLaunchKernelGGL(k_exec_adds_level, dim3((uint32_t)((g.n_adds + 255) / 256)), dim3(256), 0, s, e->tmp, e->a,
                               e->b, e->c, e->d, e->dst, (uint32_t)g.first_add, (uint32_t)g.n_adds);
            prof_end("k_exec_adds_level", 52.0 * (double)g.n_adds, s);
            if ((rc = check_launch("k_exec_adds_level"))) return rc;
        } else {
            // as many waves as the widest level needs: the barrier costs by the wave
            const uint32_t threads = (g.max_width + 63) / 64 * 64;
            hipLaunchKernelGGL(k_exec_adds_tail, dim3(1), dim3(threads), 0, s, e->tmp, e->a, e->b, e->c, e->d, e->dst,
                               e->level_end, (uint32_t)g.first_add, g.first_level, g.n_levels);
            prof_end("k_exec_adds_tail", 52.0 * (double)g.n_adds, s);
            if ((rc = check_launch("k_exec_adds_tail"))) return rc;
        }
    }
    if (!n) return 0;
    const uint64_t want = (n + 255) / 256;
    const uint32_t blocks = want < (1u << 16) ? (uint32_t)want : 1u << 16;
    // (grid y: one column each, at most 65535)
    for (uint32_t j0 = 0; j0 < P.n_cols; j0 += 65535u) {
        const uint32_t nc = P.n_cols - j0 < 65535u ? P.n_cols - j0 : 65535u;
        prof_begin(s);
        hipLaunchKernelGGL(k_exec_gather, dim3(blocks, nc), dim3(256), 0, s, cols + (uint64_t)j0 * ld, ld, n, e->tmp,
                           e->smap_t + (uint64_t)j0 * P.n_smap, P.n_smap);
        prof_end("k_exec_gather", (8.0 * (double)n + 12.0 * (double)P.n_smap) * nc, s);
        if ((rc = check_launch("k_exec_gather"))) return rc;
    }
    return 0;
}

extern "C" void zkgpu_exec_destroy(void *exec)
{
    if (!exec) return;
    Exec *e = (Exec *)exec;
    if (e->blob) {
        (void)hipStreamSynchronize(ctx().stream);  // a queued commit still reads the tables
        (void)hipFree(e->blob);
    }
    delete e;
}
