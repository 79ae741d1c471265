// The plan of a circom .exec hand-off (zkgpu_exec_*, include/zkgpu.h): the
// reference's Circom*::getCommitedPols loop (main.recursive1.cpp:343-394),
//     tmp[0 .. sizeWitness)  = the witness
//     tmp[sizeWitness + i]   = tmp[idx_1] * c + tmp[idx_2] * d         i < nAdds
//     col_j[i]               = sMap[nCols i + j] ? tmp[sMap[nCols i + j]] : 0
// validated, levelled and laid out for the GPU.  Plain host C++, no HIP: the
// library (csrc/exec.hip) and tests/cpp/exec_plan_check.cpp link it.
//
// Level schedule.  Witness slots have level 0, an add has level 1 + the
// highest level among its operands, so the adds of one level read only slots
// of lower levels and run in any order.  The adds are sorted by level
// (stably: within a level they keep the file's order) into SoA tables; each
// keeps its own result slot sizeWitness + i.  The launch plan is a list of
// segments in level order: a level wider than T adds is one grid launch; a
// run of consecutive levels of at most T adds each is one single-workgroup
// launch that walks its levels with a workgroup barrier between them (a real
// circuit's depth is its longest linear combination: one launch per level
// would leave deep narrow tails bound by the host's launch rate).  Nothing
// waits across workgroups.
#pragma once
#include <cstdint>
#include <vector>

namespace zk {

constexpr uint32_t EXEC_TAIL_MAX = 1024;  // one workgroup's threads: the widest level a tail launch takes

struct ExecSegment {
    uint32_t grid;         // 1: one level over the grid; 0: a run of narrow levels in one workgroup
    uint32_t first_level;  // index into level_end (level first_level + 1 of the schedule)
    uint32_t n_levels;
    uint32_t max_width;  // the widest level of the segment
    uint64_t first_add;  // position in the sorted tables
    uint64_t n_adds;
};

struct ExecPlan {
    uint64_t n_adds = 0, n_smap = 0, size_witness = 0;
    uint32_t n_cols = 0, n_levels = 0, tail_width = 0;
    // the adds sorted by level: tmp[dst] = tmp[a] * c + tmp[b] * d
    std::vector<uint32_t> a, b, dst;
    std::vector<uint64_t> c, d;
    std::vector<uint32_t> level;      // per add in FILE order, >= 1
    std::vector<uint32_t> level_end;  // n_levels entries: the sorted position one past level k + 1's last add
    std::vector<ExecSegment> segs;
    std::vector<uint32_t> smap_t;  // column-major: smap_t[j * n_smap + i] = sMap[n_cols * i + j]
};

// image: [nAdds, nSMap, adds[4 nAdds], sMap[nSMap n_cols]] (execFile.hpp:48-64).
// tail_width: T above, 1 .. EXEC_TAIL_MAX (0: EXEC_TAIL_MAX).  Returns 0, or
// ZKGPU_ERR_ARG with a message that names the offending add or cell.
int exec_plan_build(ExecPlan &plan, const uint64_t *image, uint64_t image_words, uint64_t size_witness,
                    uint32_t n_cols, uint32_t tail_width);

}  // namespace zk
