// zk::exec_plan_build (csrc/exec_plan.cpp) as plain host code under the host
// sanitizers: tests/test_cpp_exec_plan.py links the planner with this file
// (-fsanitize=address,undefined) and compares the lines printed here.
//
// Accepted images: every add's level equals a recomputation that relaxes
// the whole add list until nothing changes; the sorted tables are the image's
// adds, each once, at its own slot, in file order within a level; walking the
// segments level by level, every add reads only slots the witness or an
// earlier level wrote; the segments tile the levels as the rule says (a
// level wider than T alone, narrower neighbours together); sMap comes back
// transposed.  Refused images: the planner's message.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/zkgpu.h"
#include "../../zkevm-prover_amd/csrc/exec_plan.hpp"

static char g_msg[512];
namespace zk {
int set_error(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_msg, sizeof g_msg, fmt, ap);
    va_end(ap);
    return code;
}
}  // namespace zk

typedef std::vector<uint64_t> Image;
static const uint64_t P = 0xFFFFFFFF00000001ULL;
static const uint32_t T = zk::EXEC_TAIL_MAX;

static uint64_t g_s = 88172645463325252ULL;
static uint64_t rnd()
{
    g_s ^= g_s << 13;
    g_s ^= g_s >> 7;
    g_s ^= g_s << 17;
    return g_s;
}
static uint64_t word()
{
    static const uint64_t edge[6] = {0, 1, P - 1, P, P + 1, UINT64_MAX};
    const uint64_t r = rnd();
    return (r & 1) ? edge[(r >> 1) % 6] : rnd();
}

struct Adds {
    std::vector<uint64_t> w;
    uint64_t n() const { return w.size() / 4; }
    void add(uint64_t a, uint64_t b)
    {
        w.push_back(a);
        w.push_back(b);
        w.push_back(word());
        w.push_back(word());
    }
};

static Image image(const Adds &A, uint64_t sw, uint64_t n_smap, uint32_t n_cols)
{
    Image im = {A.n(), n_smap};
    im.insert(im.end(), A.w.begin(), A.w.end());
    for (uint64_t k = 0; k < n_smap * n_cols; k++) im.push_back(rnd() % 10 ? rnd() % (sw + A.n()) : 0);
    return im;
}

static std::string verify(const zk::ExecPlan &pl, const Image &im, uint64_t sw, uint32_t n_cols, uint32_t tail)
{
    const uint64_t na = im[0], ns = im[1];
    const uint64_t *adds = im.data() + 2, *smap = adds + 4 * na;
    char buf[256];
    if (pl.n_adds != na || pl.n_smap != ns || pl.size_witness != sw || pl.n_cols != n_cols) return "counts differ";
    // levels by relaxation over the whole list until a fixed point
    std::vector<uint32_t> lev(na, 1);
    for (bool moved = true; moved;) {
        moved = false;
        for (uint64_t i = na; i-- > 0;) {
            uint32_t l = 1;
            for (int k = 0; k < 2; k++)
                if (adds[4 * i + k] >= sw && lev[adds[4 * i + k] - sw] + 1 > l) l = lev[adds[4 * i + k] - sw] + 1;
            if (l != lev[i]) lev[i] = l, moved = true;
        }
    }
    uint32_t depth = 0;
    for (uint64_t i = 0; i < na; i++) {
        if (pl.level[i] != lev[i]) {
            snprintf(buf, sizeof buf, "add %llu has level %u, the relaxation gives %u", (unsigned long long)i, pl.level[i], lev[i]);
            return buf;
        }
        if (lev[i] > depth) depth = lev[i];
    }
    if (pl.n_levels != depth || pl.level_end.size() != depth) return "n_levels differs";
    if (pl.a.size() != na || pl.b.size() != na || pl.c.size() != na || pl.d.size() != na || pl.dst.size() != na)
        return "table sizes differ";
    // the segments, level by level
    std::vector<char> written(sw + na, 0);
    for (uint64_t s = 0; s < sw; s++) written[s] = 1;
    uint64_t pos = 0;
    uint32_t level = 0;
    for (size_t g = 0; g < pl.segs.size(); g++) {
        const zk::ExecSegment &sg = pl.segs[g];
        if (sg.first_add != pos || sg.first_level != level || !sg.n_levels) return "segments do not tile the schedule";
        if (sg.grid && sg.n_levels != 1) return "a grid segment of several levels";
        if (!sg.grid && g && !pl.segs[g - 1].grid) return "two tail segments in a row";
        uint32_t widest = 0;
        for (uint32_t l = 0; l < sg.n_levels; l++, level++) {
            const uint64_t end = pl.level_end[level];
            if (end < pos || end > na) return "level_end out of order";
            const uint32_t width = (uint32_t)(end - pos);
            if (!width) return "an empty level";
            if (sg.grid ? width <= tail : width > tail) return "a level in the wrong kind of segment";
            if (width > widest) widest = width;
            for (uint64_t k = pos; k < end; k++) {
                const uint64_t i = pl.dst[k] - sw;
                if (pl.dst[k] < sw || i >= na || lev[i] != level + 1) return "an add outside its level";
                if (k > pos && pl.dst[k] <= pl.dst[k - 1]) return "a level out of file order";
                if (pl.a[k] != adds[4 * i] || pl.b[k] != adds[4 * i + 1] || pl.c[k] != adds[4 * i + 2] ||
                    pl.d[k] != adds[4 * i + 3])
                    return "an add's record differs from the image";
                if (!written[pl.a[k]] || !written[pl.b[k]]) {
                    snprintf(buf, sizeof buf, "add %llu reads a slot no earlier level wrote", (unsigned long long)i);
                    return buf;
                }
            }
            for (uint64_t k = pos; k < end; k++) {
                if (written[pl.dst[k]]) return "a slot written twice";
                written[pl.dst[k]] = 1;
            }
            pos = end;
        }
        if (sg.max_width != widest || sg.n_adds != pos - sg.first_add) return "a segment's counts differ";
    }
    if (pos != na || level != depth) return "segments end early";
    if (pl.smap_t.size() != ns * n_cols) return "smap_t size differs";
    for (uint64_t i = 0; i < ns; i++)
        for (uint32_t j = 0; j < n_cols; j++)
            if (pl.smap_t[(uint64_t)j * ns + i] != smap[i * n_cols + j]) return "smap_t is not the transpose";
    return "";
}

static zk::ExecPlan g_plan;
static void run(const char *name, const Image &im, uint64_t words, uint64_t sw, uint32_t n_cols, uint32_t tail = 0)
{
    g_msg[0] = 0;
    // an exactly sized copy: the sanitizer sees any read past the stated length
    std::vector<uint64_t> exact(im.begin(), im.begin() + (words < im.size() ? words : im.size()));
    const int rc = zk::exec_plan_build(g_plan, exact.empty() ? nullptr : exact.data(), words, sw, n_cols, tail);
    if (rc) {
        printf("%s: error %d: %s\n", name, rc, g_msg);
        return;
    }
    // (the walk keeps a byte per slot: not at the 2^32 boundary)
    const std::string bad = sw >> 30 ? "" : verify(g_plan, exact, sw, n_cols, tail ? tail : T);
    if (!bad.empty()) {
        printf("%s: WRONG: %s\n", name, bad.c_str());
        return;
    }
    std::string kinds;
    for (const zk::ExecSegment &s : g_plan.segs) kinds += s.grid ? 'G' : 't';
    printf("%s: ok levels %u launches %zu %s\n", name, g_plan.n_levels, g_plan.segs.size() + 1, kinds.c_str());
}

int main()
{
    // (a) a random DAG
    Adds a;
    for (uint64_t i = 0; i < 2000; i++) a.add(i < 2 ? 0 : rnd() % (300 + i), rnd() % (300 + i));
    const Image ia = image(a, 300, 1000, 12);
    run("a_random_dag", ia, ia.size(), 300, 12);
    // (b) a chain of depth 5000
    Adds b;
    for (uint64_t i = 0; i < 5000; i++) b.add(i ? 40 + i - 1 : 3, rnd() % 40);
    const Image ib = image(b, 40, 700, 1);
    run("b_chain_5000", ib, ib.size(), 40, 1);
    if (g_plan.segs.size() + 1 > 2) printf("b_chain_5000: WRONG: more than 2 launches\n");
    // (c) wide, chain, wide
    Adds c;
    for (uint64_t i = 0; i < 70000; i++) c.add(rnd() % 500, rnd() % 500);
    for (uint64_t k = 0; k < 300; k++) c.add(500 + 70000 + k - 1, rnd() % 70500);
    for (uint64_t i = 0; i < 70000; i++) c.add(500 + 70000 + 299, rnd() % 70500);
    const Image ic = image(c, 500, 100, 18);
    run("c_grid_tail_grid", ic, ic.size(), 500, 18);
    // (d) levels of exactly T - 1, T, T + 1 adds, at the default T and at 256
    Adds d;
    for (uint32_t i = 0; i < T - 1; i++) d.add(rnd() % 64, rnd() % 64);
    for (uint32_t i = 0; i < T; i++) d.add(64 + rnd() % (T - 1), rnd() % 64);
    for (uint32_t i = 0; i < T + 1; i++) d.add(64 + T - 1 + rnd() % T, rnd() % 64);
    const Image id = image(d, 64, 0, 12);
    run("d_levels_T-1_T_T+1", id, id.size(), 64, 12);
    if (g_plan.segs.size() != 2 || g_plan.segs[0].n_levels != 2 || g_plan.segs[0].n_adds != 2 * T - 1 ||
        g_plan.segs[1].n_adds != T + 1)
        printf("d_levels_T-1_T_T+1: WRONG: not split after the level of T adds\n");
    run("d_at_tail_256", id, id.size(), 64, 12, 256);
    run("d_at_tail_1023", id, id.size(), 64, 12, T - 1);
    // (e) no adds
    const Image ie = image(Adds(), 200, 1000, 12);
    run("e_no_adds", ie, ie.size(), 200, 12);
    const Image nothing = {0, 0};
    run("e_nothing_at_all", nothing, 2, 1, 1);
    // slots up to 2^32 - 1 are accepted
    Image edge = {1, 0, 0, 4294967293ULL, 1, 1};
    run("slots_2^32-1", edge, 6, 4294967294ULL, 3);

    // ---- refusals
    run("one_word_short", ia, ia.size() - 1, 300, 12);
    Image longer = ia;
    longer.push_back(0);
    run("one_word_long", longer, longer.size(), 300, 12);
    run("another_n_cols", ia, ia.size(), 300, 13);
    run("no_header", ia, 1, 300, 12);
    const Image huge = {1ULL << 62, 0};
    run("header_that_wraps", huge, 2, 300, 12);
    Image fwd = ia;
    fwd[2 + 4 * 5 + 1] = 300 + 7;
    run("forward_reference", fwd, fwd.size(), 300, 12);
    Image self = ia;
    self[2 + 4 * 5] = 300 + 5;
    run("self_reference", self, self.size(), 300, 12);
    Image cell = ia;
    cell[2 + 4 * 2000 + 12 * 7 + 3] = 2300;
    run("smap_past_the_slots", cell, cell.size(), 300, 12);
    run("slots_2^32", edge, 6, 4294967295ULL, 3);
    run("witness_2^32", nothing, 2, 1ULL << 32, 3);
    run("no_columns", ia, ia.size(), 300, 0);
    run("no_witness", ia, ia.size(), 0, 12);
    run("tail_too_wide", ia, ia.size(), 300, 12, T + 1);
    return 0;
}
