// Host-only planner of the circom .exec hand-off: see exec_plan.hpp.
#include "exec_plan.hpp"

#include <algorithm>

#include "../../include/zkgpu.h"

namespace zk {
int set_error(int code, const char *fmt, ...);  // api.hip

typedef unsigned long long ull;

int exec_plan_build(ExecPlan &P, const uint64_t *image, uint64_t image_words, uint64_t size_witness, uint32_t n_cols,
                    uint32_t tail_width)
{
    P = ExecPlan();
    if (!n_cols) return set_error(ZKGPU_ERR_ARG, "exec_plan: n_cols is 0");
    if (!size_witness) return set_error(ZKGPU_ERR_ARG, "exec_plan: size_witness is 0");
    if (!tail_width) tail_width = EXEC_TAIL_MAX;
    if (tail_width > EXEC_TAIL_MAX)
        return set_error(ZKGPU_ERR_ARG, "exec_plan: tail width %u above %u", tail_width, EXEC_TAIL_MAX);
    if (!image || image_words < 2)
        return set_error(ZKGPU_ERR_ARG, "exec_plan: the image has %llu words, less than its 2-word header",
                         (ull)(image ? image_words : 0));
    const uint64_t n_adds = image[0], n_smap = image[1];
    const unsigned __int128 want = (unsigned __int128)2 + (unsigned __int128)4 * n_adds + (unsigned __int128)n_smap * n_cols;
    if (want != image_words)
        return set_error(ZKGPU_ERR_ARG, "exec_plan: the image has %llu words, not 2 + 4 x %llu adds + %llu x %u cells",
                         (ull)image_words, (ull)n_adds, (ull)n_smap, n_cols);
    // (n_adds < 2^62 here, so the sum cannot wrap)
    if (size_witness >= (1ULL << 32) || size_witness + n_adds >= (1ULL << 32))
        return set_error(ZKGPU_ERR_ARG, "exec_plan: size_witness + nAdds = %llu + %llu does not fit 32-bit slot indices",
                         (ull)size_witness, (ull)n_adds);
    const uint64_t n_slots = size_witness + n_adds;
    const uint64_t *adds = image + 2, *smap = adds + 4 * n_adds;

    // levels, in file order (an operand is a witness slot, level 0, or an earlier add)
    P.level.resize(n_adds);
    uint32_t n_levels = 0;
    for (uint64_t i = 0; i < n_adds; i++) {
        uint32_t lv = 0;
        for (int k = 0; k < 2; k++) {
            const uint64_t x = adds[4 * i + k];
            if (x >= size_witness + i)
                return set_error(ZKGPU_ERR_ARG, "exec_plan: add %llu reads slot %llu, not below its own slot %llu",
                                 (ull)i, (ull)x, (ull)(size_witness + i));
            if (x >= size_witness) lv = std::max(lv, P.level[x - size_witness]);
        }
        P.level[i] = lv + 1;
        n_levels = std::max(n_levels, lv + 1);
    }
    for (uint64_t i = 0; i < n_smap; i++)
        for (uint32_t j = 0; j < n_cols; j++)
            if (smap[i * n_cols + j] >= n_slots)
                return set_error(ZKGPU_ERR_ARG, "exec_plan: sMap cell (row %llu, column %u) reads slot %llu of %llu",
                                 (ull)i, j, (ull)smap[i * n_cols + j], (ull)n_slots);

    P.n_adds = n_adds;
    P.n_smap = n_smap;
    P.size_witness = size_witness;
    P.n_cols = n_cols;
    P.n_levels = n_levels;
    P.tail_width = tail_width;

    // counting sort by level: stable, so a level keeps the file's order
    P.level_end.assign(n_levels, 0);
    for (uint64_t i = 0; i < n_adds; i++) P.level_end[P.level[i] - 1]++;
    std::vector<uint32_t> pos(n_levels, 0);
    for (uint32_t l = 0, run = 0; l < n_levels; l++) {
        pos[l] = run;
        run += P.level_end[l];
        P.level_end[l] = run;
    }
    P.a.resize(n_adds);
    P.b.resize(n_adds);
    P.dst.resize(n_adds);
    P.c.resize(n_adds);
    P.d.resize(n_adds);
    for (uint64_t i = 0; i < n_adds; i++) {
        const uint32_t k = pos[P.level[i] - 1]++;
        P.a[k] = (uint32_t)adds[4 * i];
        P.b[k] = (uint32_t)adds[4 * i + 1];
        P.c[k] = adds[4 * i + 2];
        P.d[k] = adds[4 * i + 3];
        P.dst[k] = (uint32_t)(size_witness + i);
    }

    // segments: a wide level alone, a run of narrow levels together
    for (uint32_t l = 0; l < n_levels; l++) {
        const uint32_t first = l ? P.level_end[l - 1] : 0, width = P.level_end[l] - first;
        const bool wide = width > tail_width;
        if (!wide && !P.segs.empty() && !P.segs.back().grid) {
            ExecSegment &s = P.segs.back();
            s.n_levels++;
            s.n_adds += width;
            s.max_width = std::max(s.max_width, width);
        } else {
            P.segs.push_back(ExecSegment{wide ? 1u : 0u, l, 1, width, first, width});
        }
    }

    // sMap column-major: the gather's index loads and stores both run along rows
    P.smap_t.resize(n_smap * n_cols);
    for (uint64_t i = 0; i < n_smap; i++)
        for (uint32_t j = 0; j < n_cols; j++) P.smap_t[(uint64_t)j * n_smap + i] = (uint32_t)smap[i * n_cols + j];
    return 0;
}

}  // namespace zk
