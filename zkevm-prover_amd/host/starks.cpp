// libzkgpu_stark: the host-side STARK prover on top of the libzkgpu C-ABI.
//
// A C++ restatement of the reference's host orchestration -- Starks::genProof
// (src/starkpil/starks.cpp:9-404), FRIProve::prove / queryPol
// (src/starkpil/fri/friProve.cpp:5-232) and Transcript
// (src/starkpil/transcript/transcript.cpp:4-87) -- in which every bulk
// operation is a device-resident libzkgpu call on column-major sections kept
// in HBM for the whole proof.  Only roots, evals, challenges, query openings
// and the final polynomial cross PCIe.  Host arithmetic is limited to the
// scalars the reference also computes on the host (challenge transforms,
// shift powers, zhInv table size), done with the 128-bit helpers below.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <map>
#include <string>
#include <vector>

#include "../../include/zkgpu.h"
#include "../../include/zkgpu_stark.h"
#include "zkgpu_audit_format.hpp"

namespace zkgpu_host {

static thread_local char g_err[512] = "";
static int fail(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return -1;
}
// the message of the last fail() on this thread (e.g. a communicator's, before
// the prover's own wraps it)
static std::string last_error_text() { return g_err; }
#define CK(x)                                                                                                  \
    do {                                                                                                       \
        int _rc = (x);                                                                                         \
        if (_rc) return fail("%s: %s (%s:%d)", #x, zkgpu_last_error(), __FILE__, __LINE__);                   \
    } while (0)

static const uint64_t P = 0xFFFFFFFF00000001ULL;
static uint64_t mul(uint64_t a, uint64_t b) { return (uint64_t)(((unsigned __int128)a * b) % P); }
static uint64_t pw(uint64_t a, uint64_t e)
{
    uint64_t r = 1;
    a %= P;
    while (e) {
        if (e & 1) r = mul(r, a);
        a = mul(a, a);
        e >>= 1;
    }
    return r;
}
static uint64_t inv(uint64_t a) { return pw(a, P - 2); }
static uint32_t log2u(uint64_t x)  // the least k with 2^k >= x
{
    uint32_t k = 0;
    while ((1ULL << k) < x) k++;
    return k;
}
static uint64_t w_of(uint32_t n)  // Goldilocks::w(n)
{
    uint64_t w = 7277203076849721926ULL;
    for (uint32_t i = n; i < 32; i++) w = mul(w, w);
    return w;
}
static uint64_t rand_u64(uint64_t seed, uint64_t stream, uint64_t col, uint64_t row)
{
    uint64_t x = seed ^ (stream << 56) ^ (col * 0x9E3779B97F4A7C15ULL) ^ (row * 0xC2B2AE3D27D4EB4FULL);
    uint64_t z = x + 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    z ^= z >> 31;
    return z >> 1;
}

// ---------------------------------------------------------------- transcript
// The transcript runs on the host, as the reference's (transcript.cpp:4-87):
// its permutations are a serial chain on the critical path between stages, so
// they use the host permutation zkgpu_gl_poseidon_full_host (~5 us) rather
// than a single-thread GPU launch plus a synchronisation (~70 us, 90 per proof).
// Transcript (transcript.cpp:4-87)
class Transcript
{
public:
    uint64_t state[4] = {0, 0, 0, 0};
    uint64_t pending[8] = {0};
    uint64_t out[12] = {0};
    uint32_t pending_cursor = 0, out_cursor = 0;
    int err = 0;

    void absorb()
    {
        uint64_t in[12];
        memcpy(in, pending, 64);
        memcpy(in + 8, state, 32);
        if (zkgpu_gl_poseidon_full_host(out, in)) err = -1;
        out_cursor = 12;
        memset(pending, 0, sizeof pending);
        pending_cursor = 0;
        memcpy(state, out, 32);
    }
    void put(const uint64_t *v, uint64_t n)
    {
        for (uint64_t i = 0; i < n; i++) {
            pending[pending_cursor++] = v[i];
            out_cursor = 0;
            if (pending_cursor == 8) absorb();
        }
    }
    uint64_t get_fields1()
    {
        if (out_cursor == 0) absorb();
        uint64_t r = out[(12 - out_cursor) % 12];
        out_cursor--;
        return r;
    }
    void get_field(uint64_t o[3])
    {
        for (int i = 0; i < 3; i++) o[i] = get_fields1();
    }
    void get_permutations(uint64_t *res, uint64_t n, uint64_t nbits)
    {
        uint64_t nfields = (n * nbits - 1) / 63 + 1;
        std::vector<uint64_t> f(nfields);
        for (auto &x : f) x = get_fields1() % P;
        uint64_t cf = 0, cb = 0;
        for (uint64_t i = 0; i < n; i++) {
            uint64_t a = 0;
            for (uint64_t j = 0; j < nbits; j++) {
                if ((f[cf] >> cb) & 1) a |= 1ULL << j;
                if (++cb == 63) {
                    cb = 0;
                    cf++;
                }
            }
            res[i] = a;
        }
    }
};

// ---------------------------------------------------------------- prover
struct Prog {
    std::vector<zxp_instr> instr;
    std::vector<zxp_operand> opnd;
    uint32_t n_tmp1 = 0, n_tmp3 = 0;
    void set(const zkgpu_zxp_prog &p)
    {
        instr.assign(p.instr, p.instr + p.n_instr);
        opnd.assign(p.opnd, p.opnd + p.n_opnd);
        n_tmp1 = p.n_tmp1;
        n_tmp3 = p.n_tmp3;
    }
};

class Starks
{
public:
    zkgpu_stark_info info;
    std::vector<uint32_t> random_cols, zctx, ev, random_const, pu;
    std::vector<uint32_t> fri_steps;
    Prog step0, step1, step2, step3prev, step3, step42ns, step52ns;
    uint64_t N = 0, NE = 0;
    uint32_t eb = 0;
    // the n-domain rows [r0(), r0() + nb) of LEv / LpEv and evmap: all N (a rank of the sharded prover: its block)
    uint64_t nb = 0;
    virtual uint64_t r0() const { return 0; }
    zkgpu_sections S;
    std::vector<void *> allocs;
    uint64_t *nodes[4] = {nullptr, nullptr, nullptr, nullptr};
    uint64_t *const_nodes = nullptr;
    uint64_t *qq1 = nullptr, *qq2 = nullptr, *cm4_n = nullptr, *lev = nullptr, *lpev = nullptr, *xdiv = nullptr, *xdivw = nullptr;
    uint64_t *fri_pol[2] = {nullptr, nullptr};
    std::vector<uint64_t *> fri_aux, fri_nodes;
    uint64_t verkey[4];
    std::vector<uint64_t> publics;
    std::vector<std::pair<std::string, double>> timers;
    // memory plan: with `dry` set, dalloc only adds up the bytes (no device)
    bool dry = false;
    uint64_t planned = 0;
    // ZKGPU_MEM_RESIDENT or ZKGPU_MEM_LEAN (include/zkgpu_stark.h)
    int mem_mode = ZKGPU_MEM_RESIDENT;
    bool lean() const { return mem_mode == ZKGPU_MEM_LEAN; }
    // lean plan: the arena (cm1_n at its start; cm1_2ns over it from stage 4),
    // cm1's stage-1 extension above cm1_n, and the n-domain columns no stage
    // writes (zeroed before their stage: the arena's regions are reused)
    uint64_t *arena = nullptr, *cm1_early = nullptr;
    std::vector<uint32_t> unwritten[5];
    bool cm1_consumed = false;
    // lean plan: cm1's last keep_cols extended columns, kept from stage 1 in
    // their own region (what the HBM left over by the plan holds) and copied
    // into place at stage 4 instead of being extended again; (n_cm1 -
    // keep_cols) is a multiple of 8 (the linear hash's chunks)
    uint64_t keep_cols = 0;
    uint64_t *keep = nullptr;
    bool lowered_lde_batch = false;  // choose_keep set the process-wide LDE batch (restored at destruction)

    // background hand-off of the next proof's cm1_n (set_cm1_async)
    // (up to two row pieces: a shard's rows wrap around the domain end)
    uint64_t *cm1_next = nullptr, *cm1_xfer[2] = {nullptr, nullptr};
    uint64_t xfer_bytes = 0;
    void *cm1_ticket[2] = {nullptr, nullptr};
    bool cm1_pending = false;

    // streamed stage 1 (prove_from_rows): the host rows the proof in flight
    // loads its trace from, the loader's two-half stage, and whether a load
    // that failed part-way left cm1_n without a whole trace
    const uint64_t *stream_rows = nullptr;
    int stream_register = 0;
    uint64_t *stream_stage = nullptr;
    bool cm1_broken = false;
    // a whole trace has been loaded (set_cm1 / witness / a streamed or background load): the audit's precondition
    bool cm1_loaded = false;
    // the circuit's .exec plan (set_exec) and the wall time of the last
    // set_cm1_witness no proof has reported yet (< 0: none)
    void *exec = nullptr;
    double exec_commit_ms = -1.0;

    virtual ~Starks()
    {
        if (exec) zkgpu_exec_destroy(exec);
        if (lowered_lde_batch) zkgpu_set_lde_batch_cols(0);
        for (void *t : cm1_ticket) (void)zkgpu_load_wait(t);
        probe_clear();
        if (check_dev) (void)zkgpu_dev_free(check_dev);
        if (names_dev) (void)zkgpu_dev_free(names_dev);
        for (void *p : allocs) zkgpu_dev_free(p);
    }

    int dalloc(uint64_t **p, uint64_t elems)
    {
        if (dry) {
            planned += elems * 8;
            *p = (uint64_t *)(uintptr_t)4096;  // never dereferenced: the plan allocates nothing
            return 0;
        }
        void *v = nullptr;
        CK(zkgpu_dev_malloc(&v, elems * 8));
        allocs.push_back(v);
        // zeroed, as the reference's calloc'd memory map (prover.cpp:94-116):
        // a column no stage writes reads 0, in every proof
        CK(zkgpu_memset_dev(v, 0, elems * 8));
        *p = (uint64_t *)v;
        return 0;
    }

    // HBM a prover of this description holds at its peak: its own buffers
    // (alloc), the transient setup buffers and the library's grow-only
    // workspaces (extend_pol's column batches, the NTT scratch, the
    // expression programs' segment carries, calculateH1H2's table)
    virtual uint64_t setup_bytes() const { return 0; }
    virtual uint64_t lde_cols_max() const
    {
        return std::max({info.n_cm1, info.n_cm2, info.n_cm3, info.n_const, 1u});
    }
    virtual uint64_t prog_rows_max() const { return NE; }
    // the streamed stage 1's loader stage: two halves of ~64 MB, as the row
    // loaders' (a buffer of the prover's own: the library's staging workspace
    // is shared with the host-pointer calls); 0 where the call is refused
    virtual uint64_t stream_stage_words() const
    {
        const uint64_t b = std::min<uint64_t>(std::max(info.n_cm1, 1u), 128);
        return 2 * std::min<uint64_t>(N * b, (64ULL << 20) / 8);
    }
    // at most this many columns per LDE batch (0: the library's default);
    // the sharded prover lowers it when its plan would not fit otherwise
    uint64_t lde_batch_cap = 0;
    int plan(uint64_t *bytes)
    {
        dry = true;
        planned = 0;
        const int rc = alloc();
        dry = false;
        if (rc) return -1;
        const uint64_t ntt_ws = std::max<uint64_t>(3, info.n_cm4) * NE * 8;  // ntt_dev scratch (workspace slot 1)
        const uint64_t lde_ws = zkgpu_lde_workspace_bytes(
            N, NE, lde_batch_cap ? std::min<uint64_t>(lde_cols_max(), lde_batch_cap) : lde_cols_max());
        const uint64_t prog_ws = 64ULL * prog_rows_max() * 8;  // <= 64 carried columns between program segments
        const uint64_t h1h2_ws = info.n_pu ? 32ULL * N : 0;    // 2N-slot table + counts + scan
        *bytes = planned + setup_bytes() + std::max(lde_ws, ntt_ws + zkgpu_lde_workspace_bytes(N, NE, 0)) + prog_ws +
                 h1h2_ws + 24ULL * N +  // + calculateZ scratch
                 stream_stage_words() * 8;
        planned = 0;
        return 0;
    }
    // fail loudly, before any allocation, when the plan exceeds the free HBM
    int check_budget()
    {
        uint64_t need = 0, avail = 0, total = 0;
        if (plan(&need)) return -1;
        CK(zkgpu_device_memory(&avail, &total));
        if (need > avail)
            return fail("stark_create: this prover needs %.1f GB of HBM per GPU (%u-row trace, %u/%u/%u/%u committed "
                        "columns, %u constants), the device has %.1f GB free of %.1f GB",
                        need / 1e9, (unsigned)N, info.n_cm1, info.n_cm2, info.n_cm3, info.n_cm4, info.n_const,
                        avail / 1e9, total / 1e9);
        return 0;
    }

    int create(const zkgpu_stark_info *in, uint32_t mode = ZKGPU_MEM_AUTO)
    {
        if (load(in) || choose_mode(mode) || check_budget() || alloc()) return -1;
        return build_const();
    }

    // AUTO: RESIDENT when its plan fits the free HBM, else LEAN (if the
    // programs allow it; else RESIDENT, which check_budget then refuses)
    int choose_mode(uint32_t mode)
    {
        if (mode > ZKGPU_MEM_LEAN) return fail("stark_create: unknown memory plan %u", mode);
        if (mode == ZKGPU_MEM_LEAN) {
            std::string why;
            if (!lean_ok(why)) return fail("stark_create: the lean memory plan does not apply: %s", why.c_str());
            return set_mode(ZKGPU_MEM_LEAN);
        }
        mem_mode = ZKGPU_MEM_RESIDENT;
        if (mode == ZKGPU_MEM_RESIDENT) return 0;
        uint64_t need = 0, avail = 0, total = 0;
        if (plan(&need)) return -1;
        CK(zkgpu_device_memory(&avail, &total));
        std::string why;
        if (need > avail && lean_ok(why)) return set_mode(ZKGPU_MEM_LEAN);
        return 0;
    }
    int set_mode(int m, bool device = true)
    {
        mem_mode = m;
        if (m != ZKGPU_MEM_LEAN) return 0;
        find_unwritten();
        return device ? choose_keep() : 0;
    }
    // how many of cm1's extended columns the lean plan keeps from stage 1:
    // as many as the free HBM left by the plan holds (4 GB or 2 % of the
    // device spare), ZKGPU_LEAN_KEEP_COLS overriding (tests).  When not all
    // fit, LDE batches of 32 columns instead of the default 128 at 2^24 rows
    // free 19 GB of workspace for ~144 more kept columns: the LDE rate drops
    // ~1.2 % (tools/lde_batch_ab.py, profiles/r06_lde_batch_ab.json), the
    // stage-4 re-extension loses a fifth of its columns.  The batch is a
    // process-wide setting (zkgpu_set_lde_batch_cols), restored to the
    // default when this prover is destroyed.
    int choose_keep()
    {
        const uint64_t W1 = info.n_cm1;
        keep_cols = 0;
        uint64_t want = W1;
        const char *e = getenv("ZKGPU_LEAN_KEEP_COLS");
        if (e) {
            want = std::min<uint64_t>(W1, strtoull(e, nullptr, 10));
        } else {
            uint64_t avail = 0, total = 0;
            CK(zkgpu_device_memory(&avail, &total));
            const uint64_t spare = std::max<uint64_t>(4000000000ULL, total / 50);
            auto fits = [&](uint64_t cap, uint64_t &cols) {
                uint64_t need = 0;
                lde_batch_cap = cap;
                if (plan(&need)) return -1;
                cols = avail > need + spare ? std::min<uint64_t>(W1, (avail - need - spare) / (NE * 8)) : 0;
                return 0;
            };
            if (fits(0, want)) return -1;
            uint64_t want32 = 0;
            if (want < W1 && fits(32, want32)) return -1;
            if (want < W1 && want32 > want) {
                want = want32;
                zkgpu_set_lde_batch_cols(32);
                lowered_lde_batch = true;
            } else {
                lde_batch_cap = 0;
            }
        }
        const uint64_t split = W1 - want;
        keep_cols = W1 - std::min<uint64_t>(W1, (split + 7) / 8 * 8);  // (W1 - keep) a multiple of 8
        if (W1 <= 4) keep_cols = want == W1 ? W1 : 0;
        return 0;
    }

    // The lean plan needs: stage 4/5 programs that read no n-domain section
    // but the constants (their n-domain regions are gone by then), a witness
    // program that writes cm1_n only (the other n-domain regions hold cm1's
    // stage-1 extension then), and a blowup (the in-place extensions)
    bool lean_ok(std::string &why) const
    {
        if (NE < 2 * N) {
            why = "no blowup";
            return false;
        }
        const Prog *ext[2] = {&step42ns, &step52ns};
        const char *names[2] = {"step42ns", "step52ns"};
        for (int k = 0; k < 2; k++)
            for (const zxp_operand &o : ext[k]->opnd)
                if ((o.kind == ZXP_COL || o.kind == ZXP_COL3) && o.a < SEC_CONST_N) {
                    why = std::string(names[k]) + " reads an n-domain section";
                    return false;
                }
        for (const zxp_instr &i : step1.instr) {
            if (i.dst >= step1.opnd.size()) continue;
            const zxp_operand &o = step1.opnd[i.dst];
            if ((o.kind == ZXP_COL || o.kind == ZXP_COL3) && o.a != SEC_CM1_N) {
                why = "the witness program writes outside cm1_n";
                return false;
            }
        }
        return true;
    }

    // n-domain columns of tmpExp / cm2 / cm3 that no stage writes: step2,
    // calculateH1H2's h1 / h2, step3prev, calculateZ's z, step3
    void find_unwritten()
    {
        const uint32_t widths[5] = {info.n_cm1, info.n_cm2, info.n_cm3, info.n_tmp, info.n_const};
        std::vector<char> w[5];
        for (int s = 0; s < 5; s++) w[s].assign(widths[s], 0);
        for (const Prog *p : {&step2, &step3prev, &step3})
            for (const zxp_instr &i : p->instr) {
                if (i.dst >= p->opnd.size()) continue;
                const zxp_operand &o = p->opnd[i.dst];
                if ((o.kind != ZXP_COL && o.kind != ZXP_COL3) || o.a > SEC_CONST_N) continue;
                for (uint32_t c = o.b; c < o.b + (o.kind == ZXP_COL3 ? 3u : 1u) && c < widths[o.a]; c++) w[o.a][c] = 1;
            }
        for (uint32_t k = 0; k < info.n_pu; k++)
            for (uint32_t c = 0; c < pu[5 * k + 4]; c++) {
                w[SEC_CM2_N][pu[5 * k + 2] + c] = 1;
                w[SEC_CM2_N][pu[5 * k + 3] + c] = 1;
            }
        for (uint32_t z = 0; z < info.n_zctx; z++)
            for (uint32_t c = 0; c < 3; c++) w[SEC_CM3_N][zctx[3 * z + 2] + c] = 1;
        for (int s : {(int)SEC_CM2_N, (int)SEC_CM3_N, (int)SEC_TMP_N}) {
            unwritten[s].clear();
            for (uint32_t c = 0; c < widths[s]; c++)
                if (!w[s][c]) unwritten[s].push_back(c);
        }
    }
    int zero_unwritten(uint32_t s)
    {
        for (uint32_t c : unwritten[s]) CK(zkgpu_memset_dev(S.sec[s] + (uint64_t)c * N, 0, N * 8));
        return 0;
    }

    // validate the description, keep the programs, bind the device (init =
    // false: the memory plan only, no GPU)
    int load(const zkgpu_stark_info *in, bool init = true)
    {
        info = *in;
        random_cols.assign(in->random_cols, in->random_cols + in->n_random_cols);
        if (in->n_bits_ext < in->n_bits || in->n_bits_ext > 28 || in->n_fri_steps == 0 || in->n_fri_steps > 32 ||
            in->fri_steps[0] != in->n_bits_ext || in->q_deg == 0 || in->q_deg * 3 != in->n_cm4 ||
            ((uint64_t)in->q_deg << in->n_bits) > (1ULL << in->n_bits_ext) || in->l_first >= in->n_const)
            return fail("stark_create: inconsistent instance description");
        zctx.assign(in->zctx, in->zctx + 3 * in->n_zctx);
        ev.assign(in->ev, in->ev + 4 * in->n_ev);
        fri_steps.assign(in->fri_steps, in->fri_steps + in->n_fri_steps);
        if (in->n_random_const)
            random_const.assign(in->random_const, in->random_const + in->n_random_const);
        else
            for (uint32_t k = 0; k < in->n_k; k++) random_const.push_back(k);
        pu.assign(in->pu, in->pu + 5 * in->n_pu);
        for (uint32_t k = 0; k < in->n_pu; k++) {
            const uint32_t *q = &pu[5 * k];
            const uint32_t d = q[4];
            if ((d != 1 && d != 3) || q[0] + d > in->n_tmp || q[1] + d > in->n_tmp || q[2] + d > in->n_cm2 ||
                q[3] + d > in->n_cm2)
                return fail("stark_create: plookup %u out of range", k);
        }
        for (uint32_t c : random_const)
            if (c >= in->n_const) return fail("stark_create: random const column %u out of range", c);
        for (uint32_t c : random_cols)
            if (c >= in->n_cm1) return fail("stark_create: random cm1 column %u out of range", c);
        for (uint32_t z = 0; z < in->n_zctx; z++)
            if (zctx[3 * z] + 3 > in->n_tmp || zctx[3 * z + 1] + 3 > in->n_tmp || zctx[3 * z + 2] + 3 > in->n_cm3)
                return fail("stark_create: grand product %u out of range", z);
        {
            // evMap (section_2ns, col, dim, prime): starks.cpp:556-669 reads
            // pol_e[k << eb] of a 2ns section, col + dim <= its width
            const uint32_t widths_ev[5] = {in->n_cm1, in->n_cm2, in->n_cm3, in->n_cm4, in->n_const};
            for (uint32_t e = 0; e < in->n_ev; e++) {
                const uint32_t *q = &ev[4 * e];
                if (q[0] < SEC_CM1_2NS || q[0] > SEC_CONST_2NS || (q[2] != 1 && q[2] != 3) || q[3] > 1 ||
                    q[1] + q[2] > widths_ev[q[0] - SEC_CM1_2NS])
                    return fail("stark_create: evMap entry %u out of range", e);
            }
        }
        step0.set(in->step0);
        step1.set(in->step1);
        step2.set(in->step2);
        step3prev.set(in->step3prev);
        step3.set(in->step3);
        step42ns.set(in->step42ns);
        step52ns.set(in->step52ns);
        for (uint32_t si = 1; si < in->n_fri_steps; si++)
            if (in->fri_steps[si] >= in->fri_steps[si - 1] || in->fri_steps[si - 1] - in->fri_steps[si] > 5)
                return fail("stark_create: FRI steps must decrease by 1..5 bits");
        N = nb = 1ULL << in->n_bits;
        NE = 1ULL << in->n_bits_ext;
        eb = in->n_bits_ext - in->n_bits;
        if (init) CK(zkgpu_init(-1));
        return 0;
    }

    // the n-domain sections (every prover holds them whole)
    int alloc_n()
    {
        memset(&S, 0, sizeof S);
        const zkgpu_stark_info *in = &info;
        const uint32_t widths_n[5] = {in->n_cm1, in->n_cm2, in->n_cm3, in->n_tmp, in->n_const};
        for (int s = 0; s < 5; s++) {
            if (dalloc(&S.sec[s], (uint64_t)(widths_n[s] ? widths_n[s] : 1) * N)) return -1;
            S.ld[s] = N;
            S.ncols[s] = widths_n[s];
        }
        return 0;
    }

    // stage-4/5 and FRI buffers of the whole extended domain
    int alloc_fri()
    {
        // (lean: evmap reads the quotient pieces' extended rows, no cm4_n)
        if (dalloc(&qq1, 3 * NE) || dalloc(&qq2, (uint64_t)info.n_cm4 * NE) ||
            dalloc(&cm4_n, lean() ? 1 : (uint64_t)(info.n_cm4 ? info.n_cm4 : 1) * N) || dalloc(&lev, 3 * N) ||
            dalloc(&lpev, 3 * N) || dalloc(&xdiv, 3 * NE) || dalloc(&xdivw, 3 * NE) || dalloc(&fri_pol[0], 3 * NE) ||
            dalloc(&fri_pol[1], 3 * NE))
            return -1;
        fri_aux.assign(fri_steps.size(), nullptr);
        fri_nodes.assign(fri_steps.size(), nullptr);
        for (size_t si = 1; si < fri_steps.size(); si++) {
            uint64_t len = 3ULL << fri_steps[si - 1];
            if (dalloc(&fri_aux[si], len) || dalloc(&fri_nodes[si], zkgpu_gl_merkle_num_elements(1ULL << fri_steps[si])))
                return -1;
        }
        return 0;
    }

    // The lean plan (ZKGPU_MEM_LEAN): the constants, the quotient / FRI
    // buffers and the trees are held as in the resident plan; the committed
    // sections of stages 1-3 share ONE arena of (cm1 + cm2 + cm3) extended
    // columns, laid out by their lifetimes within a proof (words, e = NE / N):
    //   [0, W1 N)            cm1_n, the proof's input (set_cm1 / witness)
    //   [W1 N, W1 N + W1 NE) stage 1: cm1_2ns, hashed into tree 1, then dead
    //   [W1 N, ...)          stages 2-3: tmpExp_n, cm2_n (in (e-1) W1 N
    //                        words; appended after the arena if larger)
    //   [W1 NE, +W2 NE)      cm2_2ns from stage 2 on
    //   [(W1+W2) NE, +W3 NE) cm3_n (bottom, stage 3), then cm3_2ns extended
    //                        in place over it
    //   [0, W1 NE)           from stage 4: cm1_2ns, extended in place over
    //                        cm1_n (whose stage-1 extension was dropped)
    // The n-domain values die after the stage-3 commit: evmap reads the
    // extended rows k << blowup with the Lagrange weights of xi / 7, as the
    // reference does (starks.cpp:308-333).
    int alloc_lean()
    {
        if (alloc_fri()) return -1;
        memset(&S, 0, sizeof S);
        const uint64_t W1 = std::max(info.n_cm1, 1u), W2 = std::max(info.n_cm2, 1u), W3 = std::max(info.n_cm3, 1u),
                       WT = std::max(info.n_tmp, 1u), WC = std::max(info.n_const, 1u);
        // resident sections: constants (both domains), cm4, q, f
        if (dalloc(&S.sec[SEC_CONST_N], WC * N) || dalloc(&S.sec[SEC_CONST_2NS], WC * NE) ||
            dalloc(&S.sec[SEC_CM4_2NS], (uint64_t)std::max(info.n_cm4, 1u) * NE) ||
            dalloc(&S.sec[SEC_Q_2NS], 3 * NE) || dalloc(&S.sec[SEC_F_2NS], 3 * NE))
            return -1;
        uint64_t words = (W1 + W2 + W3) * NE;
        const uint64_t high = W1 * N, high_words = W1 * NE - W1 * N;
        uint64_t tmp_off = high;
        if ((WT + W2) * N > high_words) {
            tmp_off = words;
            words += (WT + W2) * N;
        }
        words = std::max(words, high + (W1 - keep_cols) * NE);  // cm1's stage-1 extension (not kept)
        if (dalloc(&arena, words)) return -1;
        if (keep_cols && dalloc(&keep, keep_cols * NE)) return -1;
        S.sec[SEC_CM1_N] = arena;
        S.sec[SEC_TMP_N] = arena + tmp_off;
        S.sec[SEC_CM2_N] = arena + tmp_off + WT * N;
        S.sec[SEC_CM2_2NS] = arena + W1 * NE;
        S.sec[SEC_CM3_2NS] = arena + (W1 + W2) * NE;
        S.sec[SEC_CM3_N] = S.sec[SEC_CM3_2NS];
        cm1_early = arena + high;
        S.sec[SEC_CM1_2NS] = cm1_early;
        const uint32_t widths[SEC_COUNT] = {info.n_cm1, info.n_cm2,  info.n_cm3, info.n_tmp, info.n_const, info.n_cm1,
                                            info.n_cm2, info.n_cm3, info.n_cm4, info.n_const, 3,           3};
        for (int s = 0; s < SEC_COUNT; s++) {
            S.ld[s] = s <= SEC_CONST_N ? N : NE;
            S.ncols[s] = widths[s];
        }
        uint64_t tn = zkgpu_gl_merkle_num_elements(NE);
        for (int t = 0; t < 4; t++)
            if (dalloc(&nodes[t], tn)) return -1;
        return dalloc(&const_nodes, tn);
    }

    virtual int alloc()
    {
        if (lean()) return alloc_lean();
        if (alloc_n() || alloc_fri()) return -1;
        const zkgpu_stark_info *in = &info;
        const uint32_t widths_e[7] = {in->n_cm1, in->n_cm2, in->n_cm3, in->n_cm4, in->n_const, 3, 3};
        for (int s = 0; s < 7; s++) {
            if (dalloc(&S.sec[SEC_CM1_2NS + s], (uint64_t)(widths_e[s] ? widths_e[s] : 1) * NE)) return -1;
            S.ld[SEC_CM1_2NS + s] = NE;
            S.ncols[SEC_CM1_2NS + s] = widths_e[s];
        }
        uint64_t tn = zkgpu_gl_merkle_num_elements(NE);
        for (int t = 0; t < 4; t++)
            if (dalloc(&nodes[t], tn)) return -1;
        if (dalloc(&const_nodes, tn)) return -1;
        return 0;
    }

    // constants (setup): pseudo-random columns, L_first = [1, 0, ...], then
    // step0, on the whole n domain of S.sec[SEC_CONST_N] (ld N)
    int fill_const()
    {
        const zkgpu_stark_info *in = &info;
        CK(zkgpu_memset_dev(S.sec[SEC_CONST_N], 0, (uint64_t)in->n_const * N * 8));
        if (!random_const.empty())
            CK(zkgpu_rand_cols_dev(S.sec[SEC_CONST_N], N, random_const.data(), (uint32_t)random_const.size(), N,
                                   in->seed, 1));
        uint64_t one = 1;
        CK(zkgpu_memcpy_h2d(S.sec[SEC_CONST_N] + (uint64_t)in->l_first * N, &one, 8));
        if (!step0.instr.empty()) {
            uint64_t ch0[24] = {0}, ev0[3] = {0, 0, 0};
            if (run(step0, false, ch0, ev0, 0)) return -1;
        }
        return 0;
    }
    void init_publics()
    {
        publics.resize(info.n_publics);
        for (uint32_t k = 0; k < info.n_publics; k++) publics[k] = rand_u64(info.seed, 2, k, 0);
    }
    virtual int build_const()
    {
        if (fill_const() || commit_const()) return -1;
        init_publics();
        return 0;
    }

    int run(const Prog &p, bool ext, const uint64_t ch[24], const uint64_t *evals, uint32_t n_ev)
    {
        CK(zkgpu_zxp_eval_dev(p.instr.data(), (uint32_t)p.instr.size(), p.opnd.data(), (uint32_t)p.opnd.size(),
                              p.n_tmp1 ? p.n_tmp1 : 1, p.n_tmp3 ? p.n_tmp3 : 1, &S,
                              ext ? info.n_bits_ext : info.n_bits, ch, publics.data(), (uint32_t)publics.size(),
                              evals, n_ev, ext ? xdiv : nullptr, ext ? xdivw : nullptr, eb, ext ? 7 : 1));
        return 0;
    }

    virtual int witness()
    {
        CK(zkgpu_memset_dev(S.sec[SEC_CM1_N], 0, (uint64_t)info.n_cm1 * N * 8));
        CK(zkgpu_rand_cols_dev(S.sec[SEC_CM1_N], N, random_cols.data(), (uint32_t)random_cols.size(), N, info.seed, 0));
        uint64_t ch[24] = {0};
        uint64_t ev0[3] = {0, 0, 0};
        if (run(step1, false, ch, ev0, 0)) return -1;
        CK(zkgpu_synchronize());
        cm1_consumed = cm1_broken = false;
        cm1_loaded = true;
        return 0;
    }

    // the executor's row-major buffer, streamed in row blocks (no full-size
    // staging copy: at the fork-9 widths cm1_n is 25-50 GB)
    virtual int set_cm1(const uint64_t *rows)
    {
        if (take_cm1_async(false)) return -1;  // a pending background load is superseded
        if (zkgpu_load_rows_dev(S.sec[SEC_CM1_N], N, rows, N, info.n_cm1, 0, 0))
            return fail("set_cm1: %s", zkgpu_last_error());
        cm1_consumed = cm1_broken = false;
        cm1_loaded = true;
        return 0;
    }

    // The circuit's .exec hand-off (Circom*::getCommitedPols, prover.cpp:591-593,
    // 629-630): planned for n_cm1 columns, its tables and tmp in a device block
    // of their own outside the memory plan (zkgpu_exec_info reports the
    // bytes), as the probe's block is.  A second call replaces the plan.
    virtual int set_exec(const uint64_t *image, uint64_t image_words, uint64_t size_witness)
    {
        if (!image) return fail("set_exec: null argument");
        if (!info.n_cm1) return fail("set_exec: the instance has no committed trace columns");
        void *e = nullptr;
        if (zkgpu_exec_create(&e, image, image_words, size_witness, info.n_cm1))
            return fail("set_exec: %s", zkgpu_last_error());
        uint64_t n_smap = 0;
        (void)zkgpu_exec_info(e, nullptr, &n_smap, nullptr, nullptr, nullptr);
        if (n_smap > N) {
            zkgpu_exec_destroy(e);
            return fail("set_exec: the sMap has %llu rows, the trace %llu", (unsigned long long)n_smap,
                        (unsigned long long)N);
        }
        if (exec) zkgpu_exec_destroy(exec);
        exec = e;
        return 0;
    }

    // witness -> cm1_n through the plan of set_exec: the prover is left as
    // set_cm1 of the reference's buffer leaves it
    virtual int set_cm1_witness(const uint64_t *wit)
    {
        if (!exec) return fail("set_cm1_witness: no .exec plan is set; call set_exec first");
        if (!wit) return fail("set_cm1_witness: null argument");
        if (take_cm1_async(false)) return -1;  // a pending background load is superseded
        const auto t = clk::now();
        if (zkgpu_exec_commit_dev(exec, wit, S.sec[SEC_CM1_N], N, N) || zkgpu_synchronize()) {
            cm1_broken = true;  // what the kernels reached of cm1_n is no whole trace
            cm1_loaded = false;
            return fail("set_cm1_witness: %s", zkgpu_last_error());
        }
        exec_commit_ms = std::chrono::duration<double, std::milli>(clk::now() - t).count();
        timers.clear();
        timers.emplace_back("ZKGPU_EXEC_COMMIT", exec_commit_ms);
        cm1_consumed = cm1_broken = false;
        cm1_loaded = true;
        return 0;
    }

    // cm1_n back as the executor's row-major layout (n rows x n_cm1)
    virtual int get_cm1(uint64_t *rows)
    {
        if (lean() && cm1_consumed) return fail("get_cm1: the last proof consumed the trace (lean memory plan)");
        if (cm1_broken) return fail("get_cm1: the last streamed load failed part-way: no whole trace is loaded");
        // in row blocks of ~256 MB (no full-size device copy: under the lean
        // plan a second cm1_n does not fit beside the arena)
        void *tmp = nullptr;
        const uint64_t W1 = info.n_cm1;
        const uint64_t blk = std::min<uint64_t>(N, std::max<uint64_t>(1, (256ULL << 20) / (std::max<uint64_t>(W1, 1) * 8)));
        CK(zkgpu_dev_malloc(&tmp, std::max<uint64_t>(8, blk * W1 * 8)));
        int rc = 0;
        for (uint64_t r0 = 0; r0 < N && W1 && !rc; r0 += blk) {
            const uint64_t nr = std::min(blk, N - r0);
            rc = zkgpu_cols_to_rows_dev((uint64_t *)tmp, S.sec[SEC_CM1_N] + r0, N, nr, W1);
            if (!rc) rc = zkgpu_memcpy_d2h(rows + r0 * W1, tmp, nr * W1 * 8);
        }
        zkgpu_dev_free(tmp);
        if (rc) return fail("get_cm1: %s", zkgpu_last_error());
        return 0;
    }

    virtual int set_cm1_async(const uint64_t *rows)
    {
        if (lean())
            return fail("set_cm1_async: not offered under the lean memory plan (the proof extends cm1_n in place; "
                        "the next trace's buffer would not fit beside it); use set_cm1 between proofs");
        if (take_cm1_async(false)) return -1;
        if (cm1_next_alloc(N, 1)) return -1;
        if (zkgpu_load_rows_async(cm1_next, N, rows, N, info.n_cm1, 0, cm1_xfer[0], xfer_bytes, &cm1_ticket[0]))
            return fail("set_cm1_async: %s", zkgpu_last_error());
        cm1_pending = true;
        return 0;
    }

    // the second cm1_n buffer (ld rows per column) and `pieces` loader stages
    int cm1_next_alloc(uint64_t ld, int pieces)
    {
        if (cm1_next) return 0;
        xfer_bytes = zkgpu_load_rows_stage_bytes(ld, info.n_cm1, 0);
        if (dalloc(&cm1_next, (uint64_t)(info.n_cm1 ? info.n_cm1 : 1) * ld)) return -1;
        for (int k = 0; k < pieces; k++)
            if (dalloc(&cm1_xfer[k], std::max<uint64_t>(1, xfer_bytes / 8))) return -1;
        return 0;
    }

    // wait for a queued background load; with `use`, swap its buffer in as
    // cm1_n (every consumer reads S.sec at call time), else drop it
    int take_cm1_async(bool use)
    {
        if (!cm1_pending) return 0;
        cm1_pending = false;
        int rc = 0;
        for (void *&t : cm1_ticket) {
            const int r = zkgpu_load_wait(t);
            t = nullptr;
            rc = rc ? rc : r;
        }
        if (rc) return fail("set_cm1_async: %s", zkgpu_last_error());
        if (use) {
            std::swap(S.sec[SEC_CM1_N], cm1_next);
            cm1_loaded = true;
        }
        return 0;
    }

    // constant polynomials from the reference's .const file layout (N rows x
    // nConstants, ConstantPolsStarks, starks.hpp:94-116), their LDE and tree
    virtual int set_const(const uint64_t *rows)
    {
        void *tmp = nullptr;
        CK(zkgpu_dev_malloc(&tmp, (uint64_t)(info.n_const ? info.n_const : 1) * N * 8));
        int rc = zkgpu_memcpy_h2d(tmp, rows, (uint64_t)info.n_const * N * 8);
        if (!rc) rc = zkgpu_rows_to_cols_dev(S.sec[SEC_CONST_N], N, (const uint64_t *)tmp, N, info.n_const);
        if (!rc) rc = zkgpu_synchronize();
        zkgpu_dev_free(tmp);
        if (rc) return fail("set_const: %s", zkgpu_last_error());
        return commit_const();
    }

    // LDE of the constant polynomials, their tree, verkey = its root
    virtual int commit_const()
    {
        CK(zkgpu_gl_extend_pol_dev(S.sec[SEC_CONST_2NS], NE, S.sec[SEC_CONST_N], N, NE, N, info.n_const));
        CK(zkgpu_gl_merkletree_dev(const_nodes, S.sec[SEC_CONST_2NS], NE, info.n_const, NE));
        CK(zkgpu_memcpy_d2h(verkey, const_nodes + zkgpu_gl_merkle_num_elements(NE) - 4, 32));
        return 0;
    }

    int set_publics(const uint64_t *p)
    {
        for (uint32_t k = 0; k < info.n_publics; k++) publics[k] = p[k] % P;
        return 0;
    }

    uint32_t q() const { return info.n_queries; }

    uint64_t proof_len() const
    {
        uint64_t L = 16 + 3ULL * info.n_ev;
        for (size_t si = 1; si < fri_steps.size(); si++)
            L += 4 + (uint64_t)q() * (3ULL << (fri_steps[si - 1] - fri_steps[si])) + (uint64_t)q() * fri_steps[si] * 4;
        L += (uint64_t)q() * (info.n_cm1 + info.n_cm2 + info.n_cm3 + info.n_cm4 + info.n_const);
        L += 5ULL * q() * info.n_bits_ext * 4;
        L += 3ULL << fri_steps.back();
        return L;
    }

    // Stage timers (the reference's TimerStart / TimerStopAndLog) between
    // stream marks, resolved once at the end of the proof (flush_timers): a
    // stage boundary costs no device synchronisation (config-4: ~20 per
    // proof, each a dependent launch's gap); the synchronous form only when
    // the mark pool is spent
    using clk = std::chrono::steady_clock;
    clk::time_point t0;
    uint32_t t0_mark = UINT32_MAX, n_marks = 0;
    std::vector<std::pair<size_t, std::pair<uint32_t, uint32_t>>> pend_t;  // timer index, marks
    void tstart()
    {
        t0 = clk::now();
        t0_mark = UINT32_MAX;
        if (n_marks + 1 < ZKGPU_MARKS && !zkgpu_mark(n_marks)) t0_mark = n_marks++;
    }
    // ZKGPU_SYNC_STAGES=1 (debugging): a device synchronisation at every
    // stage end, so an asynchronous kernel fault is reported by the stage
    // that launched it rather than at the proof's end (flush_timers)
    bool sync_stages = [] {
        const char *e = getenv("ZKGPU_SYNC_STAGES");
        return e && atoi(e) != 0;
    }();
    int tstop(const char *name)
    {
        if (sync_stages && zkgpu_synchronize()) return fail("%s: %s", name, zkgpu_last_error());
        if (t0_mark != UINT32_MAX && n_marks < ZKGPU_MARKS && !zkgpu_mark(n_marks)) {
            pend_t.push_back({timers.size(), {t0_mark, n_marks++}});
            timers.emplace_back(name, 0.0);
            return 0;
        }
        CK(zkgpu_synchronize());
        timers.emplace_back(name, std::chrono::duration<double, std::milli>(clk::now() - t0).count());
        return 0;
    }
    // a commit's timers, STARK_STEP_<stage>_<what>; stage 0 (the constants'
    // commit, outside any proof): no timer
    int tstop_commit(int stage, const char *what)
    {
        return stage ? tstop(("STARK_STEP_" + std::to_string(stage) + "_" + what).c_str()) : 0;
    }
    // exchanges of a sharded proof: (marks, bytes sent) -> the total device
    // time inside them and that of the largest one
    std::vector<std::pair<std::pair<uint32_t, uint32_t>, uint64_t>> pend_x;
    double xchg_ms = 0, xchg_max_ms = 0;
    int flush_timers()
    {
        for (const auto &p : pend_t) {
            double ms = 0;
            CK(zkgpu_mark_elapsed(p.second.first, p.second.second, &ms));
            timers[p.first].second = ms;
        }
        pend_t.clear();
        xchg_ms = xchg_max_ms = 0;
        uint64_t big = 0;
        for (const auto &x : pend_x) {
            double ms = 0;
            CK(zkgpu_mark_elapsed(x.first.first, x.first.second, &ms));
            xchg_ms += ms;
            if (x.second >= big) {
                big = x.second;
                xchg_max_ms = ms;
            }
        }
        pend_x.clear();
        n_marks = 0;
        t0_mark = UINT32_MAX;
        return 0;
    }

    // the committed columns of stage t = 1 .. 4 (cm1 .. cm4), sections
    // SEC_CM1_2NS + t - 1 and, for t < 4, SEC_CM1_N + t - 1
    uint32_t stage_cols(int t) const
    {
        const uint32_t w[4] = {info.n_cm1, info.n_cm2, info.n_cm3, info.n_cm4};
        return w[t - 1];
    }

    // lean plan, stage 1: cm1's extension into the scratch above cm1_n
    // (columns [0, split), hashed and dropped) and into `keep` (the rest,
    // kept for stage 4), one tree over both regions
    int commit_cm1_lean(uint64_t root[4])
    {
        const uint64_t W1 = info.n_cm1, split = W1 - keep_cols;
        S.sec[SEC_CM1_2NS] = cm1_early;
        tstart();
        if (split) CK(zkgpu_gl_extend_pol_dev(cm1_early, NE, arena, N, NE, N, split));
        if (keep_cols) CK(zkgpu_gl_extend_pol_dev(keep, NE, arena + split * N, N, NE, N, keep_cols));
        if (tstop_commit(1, "LDE")) return -1;
        tstart();
        if (!keep_cols)
            CK(zkgpu_gl_merkletree_dev(nodes[0], cm1_early, NE, W1, NE));
        else if (!split)
            CK(zkgpu_gl_merkletree_dev(nodes[0], keep, NE, W1, NE));
        else
            CK(zkgpu_gl_merkletree2_dev(nodes[0], cm1_early, keep, NE, split, W1, NE));
        CK(zkgpu_memcpy_d2h(root, nodes[0] + zkgpu_gl_merkle_num_elements(NE) - 4, 32));
        return tstop_commit(1, "MERKLETREE");
    }

    // columns per batch of the streamed stage 1, a multiple of 8 (the linear
    // hash's blocks): 128, the LDE's default column batch, for a wide trace --
    // the strided block copies move 1 KB per row at 52 GB/s, 256 B per row (32
    // columns) at 37 GB/s, and the copy is what bounds stage 1 (2^23 rows x
    // 751 columns: 1.12 s at 128, 1.38 s at 32; extend_pol splits a batch into
    // its own LDE batches where the plan lowered those) -- and 64 below 256
    // columns, where a 128-column batch would leave nothing to overlap (2^23
    // rows x 100 columns: 217 ms at 64, 246 ms in one batch).  Measured by
    // tools/handoff_stream_ab.py (profiles/r07_handoff_stream.json).
    // ZKGPU_STREAM_COLS overrides (tests).
    uint64_t stream_batch_cols() const
    {
        uint64_t b = info.n_cm1 >= 256 ? 128 : 64;
        const char *e = getenv("ZKGPU_STREAM_COLS");
        if (e && *e) b = strtoull(e, nullptr, 10);
        return std::max<uint64_t>(8, (b + 7) / 8 * 8);
    }

    // stage 1 of prove_from_rows: the trace crosses PCIe in column batches,
    // each into its final place in cm1_n; the library stream waits for a
    // batch, extends it (resident: into cm1_2ns; lean: into the scratch above
    // cm1_n up to `split`, into `keep` from there, as commit_cm1_lean) and
    // absorbs it into tree 1's leaf sponge while the later batches load.
    // Loads and compute are queued from this one thread: every wait is queued
    // after the record it waits for.  A failure leaves cm1_broken set.
    int commit_cm1_stream(uint64_t root[4])
    {
        const uint64_t W1 = info.n_cm1, split = lean() ? W1 - keep_cols : W1, B = stream_batch_cols();
        if (lean()) S.sec[SEC_CM1_2NS] = cm1_early;
        uint64_t *ext_lo = S.sec[SEC_CM1_2NS];
        if (!stream_stage && dalloc(&stream_stage, stream_stage_words())) return -1;
        cm1_broken = true;
        cm1_consumed = false;
        tstart();
        void *loader = nullptr;
        if (zkgpu_load_stream_open(&loader, stream_rows, N, W1, stream_stage, stream_stage_words() * 8,
                                   stream_register))
            return fail("prove_from_rows: %s", zkgpu_last_error());
        int rc = 0;
        for (uint64_t c0 = 0; c0 < W1 && !rc;) {
            uint64_t nc = std::min(B, W1 - c0);
            if (c0 < split && c0 + nc > split) nc = split - c0;  // no batch straddles the two regions
            uint64_t *cn = S.sec[SEC_CM1_N] + c0 * N;
            uint64_t *ce = c0 < split ? ext_lo + c0 * NE : keep + (c0 - split) * NE;
            rc = zkgpu_load_stream_window(loader, cn, N, c0, nc);
            if (!rc) rc = zkgpu_gl_extend_pol_dev(ce, NE, cn, N, NE, N, nc);
            if (!rc) rc = zkgpu_gl_merkle_leaves_absorb_dev(nodes[0], ce, NE, c0, nc, W1, NE);
            c0 += nc;
        }
        if (!rc) rc = zkgpu_gl_merkle_finish_dev(nodes[0], NE);
        if (!rc) rc = zkgpu_memcpy_d2h(root, nodes[0] + zkgpu_gl_merkle_num_elements(NE) - 4, 32);
        // everything queued is drained before the call returns, failed or not
        const std::string why = rc ? zkgpu_last_error() : "";
        const int rc_close = zkgpu_load_stream_close(loader);
        if (rc) {
            (void)zkgpu_synchronize();
            return fail("prove_from_rows: %s", why.c_str());
        }
        if (rc_close) return fail("prove_from_rows: %s", zkgpu_last_error());
        cm1_broken = false;
        cm1_loaded = true;
        return tstop("STARK_STEP_1_STREAM");
    }

    // one proof of the executor's host buffer: set_cm1(rows) + prove() with
    // the upload under stage 1 (commit_cm1_stream).  A pending background
    // load is dropped, as by set_cm1.
    virtual int prove_from_rows(const uint64_t *rows, int register_host, uint64_t *out)
    {
        if (!rows || !out) return fail("prove_from_rows: null argument");
        if (!info.n_cm1) return fail("prove_from_rows: the instance has no committed trace columns");
        if (take_cm1_async(false)) return -1;
        stream_rows = rows;
        stream_register = register_host;
        const int rc = prove_body(out);
        stream_rows = nullptr;
        return rc;
    }

    // the proof of the current cm1_n; a trace queued by set_cm1_async (loaded
    // meanwhile) becomes cm1_n when it returns
    virtual int prove(uint64_t *out)
    {
        if (cm1_broken)
            return fail("stark_prove: the last streamed load (prove_from_rows) failed part-way: no whole trace is "
                        "loaded; load one with set_cm1 or witness first");
        if (lean() && cm1_consumed)
            return fail("stark_prove: the previous proof consumed the trace (lean memory plan: cm1_n is extended in "
                        "place); load the next one with set_cm1 or witness first");
        const int rc = prove_body(out);
        const int rc2 = take_cm1_async(true);
        return rc ? rc : rc2;
    }

    // ---- probe (include/zkgpu_stark.h): sampled rows of the sections around
    // every stage program.  probe_set derives the record list from the
    // programs and allocates the device block the records are gathered into;
    // prove_body's hooks (probe_point) enqueue one gather per record on the
    // prover's stream, from the section table as it stands at that moment, and
    // copy the host scalars; probe_readback brings the block to the host after
    // the proof.  Nothing here synchronises inside a proof.
    struct ProbeRec {
        zkgpu_probe_rec r;
        uint64_t rows_dev = 0;  // its row list in probe_rows (device), in words
        uint64_t stage = 0;     // its values in probe_stage (device), in words
    };
    std::vector<ProbeRec> probe_recs;
    std::vector<uint32_t> probe_at[ZKGPU_PROBE_POINTS][2];  // records of (point, after)
    std::vector<uint64_t> probe_payload;  // row lists and scalars, then the image of probe_stage
    uint64_t probe_gather0 = 0, probe_stage_words = 0;
    uint64_t *probe_stage = nullptr, *probe_rows = nullptr;
    bool probe_valid = false;

    void probe_clear()
    {
        if (probe_stage) (void)zkgpu_dev_free(probe_stage);
        if (probe_rows) (void)zkgpu_dev_free(probe_rows);
        probe_stage = probe_rows = nullptr;
        probe_recs.clear();
        for (auto &pt : probe_at)
            for (auto &v : pt) v.clear();
        probe_payload.clear();
        probe_gather0 = probe_stage_words = 0;
        probe_valid = false;
    }

    virtual int probe_set(const uint64_t *rows_n, uint32_t n_rows_n, const uint64_t *rows_ext, uint32_t n_rows_ext)
    {
        probe_clear();
        if (!n_rows_n && !n_rows_ext) return 0;
        if ((n_rows_n && !rows_n) || (n_rows_ext && !rows_ext)) return fail("probe_set: null row list");
        if (n_rows_n > ZKGPU_PROBE_MAX_ROWS || n_rows_ext > ZKGPU_PROBE_MAX_ROWS)
            return fail("probe_set: %u / %u sampled rows, at most %u per domain", n_rows_n, n_rows_ext,
                        ZKGPU_PROBE_MAX_ROWS);
        std::vector<uint64_t> base[2] = {std::vector<uint64_t>(rows_n, rows_n + n_rows_n),
                                         std::vector<uint64_t>(rows_ext, rows_ext + n_rows_ext)};
        for (int e = 0; e < 2; e++) {
            std::sort(base[e].begin(), base[e].end());
            base[e].erase(std::unique(base[e].begin(), base[e].end()), base[e].end());
            const uint64_t dom = e ? NE : N;
            if (!base[e].empty() && base[e].back() >= dom)
                return fail("probe_set: row %llu is outside the %s domain (%llu rows)",
                            (unsigned long long)base[e].back(), e ? "extended" : "n", (unsigned long long)dom);
        }
        std::vector<std::vector<uint64_t>> lists;  // row list of each record
        auto add = [&](uint32_t point, uint32_t after, uint32_t sec, uint32_t ncols, std::vector<uint64_t> rows) {
            ProbeRec p;
            p.r = {point, after, sec, ncols, (uint64_t)rows.size(), 0, 0};
            probe_at[point][after].push_back((uint32_t)probe_recs.size());
            probe_recs.push_back(p);
            lists.push_back(std::move(rows));
        };
        const uint32_t n_scal = 24 + 3 * info.n_ev;
        struct Point {
            uint32_t point;
            const Prog *prog;  // null: a stage step with one after-record
            bool ext, present;
            uint32_t sec;
            const char *name;
        };
        const Point points[ZKGPU_PROBE_POINTS] = {
            {ZKGPU_PROBE_STEP2, &step2, false, true, 0, "step2"},
            {ZKGPU_PROBE_H1H2, nullptr, false, info.n_pu != 0, SEC_CM2_N, "h1h2"},
            {ZKGPU_PROBE_STEP3PREV, &step3prev, false, true, 0, "step3prev"},
            {ZKGPU_PROBE_Z, nullptr, false, true, SEC_CM3_N, "z"},
            {ZKGPU_PROBE_STEP3, &step3, false, !step3.instr.empty(), 0, "step3"},
            {ZKGPU_PROBE_STEP42NS, &step42ns, true, true, 0, "step42ns"},
            {ZKGPU_PROBE_QSPLIT, nullptr, true, true, SEC_CM4_2NS, "qsplit"},
            {ZKGPU_PROBE_STEP52NS, &step52ns, true, true, 0, "step52ns"},
        };
        for (const Point &pt : points) {
            if (!pt.present) continue;
            add(pt.point, 0, ZKGPU_PROBE_SCALARS, n_scal, {0});
            const uint64_t dom = pt.ext ? NE : N;
            if (!pt.prog) {
                add(pt.point, 1, pt.sec, S.ncols[pt.sec], base[pt.ext]);
                continue;
            }
            // the sections the program reads / stores to, and every row shift it uses with each
            std::vector<int32_t> shifts[SEC_COUNT];
            bool reads[SEC_COUNT] = {false}, stores[SEC_COUNT] = {false};
            auto use = [&](uint32_t k, bool store) -> int {
                if (k >= pt.prog->opnd.size()) return fail("probe_set: %s names operand %u of %zu", pt.name, k,
                                                           pt.prog->opnd.size());
                const zxp_operand &o = pt.prog->opnd[k];
                if (o.kind != ZXP_COL && o.kind != ZXP_COL3) return 0;
                if (o.a >= SEC_COUNT) return fail("probe_set: %s names section %u", pt.name, o.a);
                if ((o.a >= SEC_CM1_2NS) != pt.ext)
                    return fail("probe_set: %s %s section %u of the other domain: its rows are not the sampled rows'",
                                pt.name, store ? "writes" : "reads", o.a);
                (store ? stores : reads)[o.a] = true;
                shifts[o.a].push_back((int32_t)o.c);
                return 0;
            };
            for (const zxp_instr &in : pt.prog->instr)
                if (use(in.a, false) || (in.op != ZXP_COPY && use(in.b, false)) || use(in.dst, true)) {
                    probe_clear();
                    return -1;
                }
            std::vector<uint64_t> rows[SEC_COUNT];
            for (uint32_t s = 0; s < SEC_COUNT; s++) {
                if (!reads[s] && !stores[s]) continue;
                shifts[s].push_back(0);
                for (uint64_t r : base[pt.ext])
                    for (int32_t sh : shifts[s]) rows[s].push_back((r + (uint64_t)(int64_t)sh) & (dom - 1));
                std::sort(rows[s].begin(), rows[s].end());
                rows[s].erase(std::unique(rows[s].begin(), rows[s].end()), rows[s].end());
            }
            for (uint32_t after = 0; after < 2; after++)
                for (uint32_t s = 0; s < SEC_COUNT; s++)
                    if (after ? stores[s] : reads[s]) add(pt.point, after, s, S.ncols[s], rows[s]);
        }
        // payload: every record's row list (and the scalars' values), then the gathered values
        uint64_t cur = 0;
        for (size_t i = 0; i < probe_recs.size(); i++) {
            zkgpu_probe_rec &r = probe_recs[i].r;
            r.rows_off = cur;
            cur += r.n_rows;
            if (r.section == ZKGPU_PROBE_SCALARS) {
                r.vals_off = cur;
                cur += r.ncols;
            }
        }
        probe_gather0 = cur;
        std::map<std::vector<uint64_t>, uint64_t> seen;  // identical row lists share one device copy
        std::vector<uint64_t> dev_rows;
        for (size_t i = 0; i < probe_recs.size(); i++) {
            ProbeRec &p = probe_recs[i];
            if (p.r.section == ZKGPU_PROBE_SCALARS) continue;
            p.stage = probe_stage_words;
            p.r.vals_off = probe_gather0 + probe_stage_words;
            probe_stage_words += p.r.n_rows * p.r.ncols;
            auto it = seen.find(lists[i]);
            if (it == seen.end()) {
                it = seen.emplace(lists[i], (uint64_t)dev_rows.size()).first;
                dev_rows.insert(dev_rows.end(), lists[i].begin(), lists[i].end());
            }
            p.rows_dev = it->second;
        }
        probe_payload.assign(probe_gather0 + probe_stage_words, 0);
        for (size_t i = 0; i < probe_recs.size(); i++)
            std::copy(lists[i].begin(), lists[i].end(), probe_payload.begin() + probe_recs[i].r.rows_off);
        void *stage = nullptr, *rows = nullptr;
        if (zkgpu_dev_malloc(&stage, probe_stage_words * 8) || zkgpu_dev_malloc(&rows, dev_rows.size() * 8)) {
            if (stage) (void)zkgpu_dev_free(stage);
            const double mb = (double)(probe_stage_words + dev_rows.size()) * 8 / 1e6;
            probe_clear();
            return fail("probe_set: the probe's device block (%.1f MB) could not be allocated: %s; the probe is off",
                        mb, zkgpu_last_error());
        }
        probe_stage = (uint64_t *)stage;
        probe_rows = (uint64_t *)rows;
        if (zkgpu_memcpy_h2d(probe_rows, dev_rows.data(), dev_rows.size() * 8)) {
            probe_clear();
            return fail("probe_set: %s; the probe is off", zkgpu_last_error());
        }
        return 0;
    }

    // the records of (point, after): the scalars from the host, every section from the live table
    int probe_point(uint32_t point, uint32_t after, const uint64_t ch[24], const std::vector<uint64_t> &evals)
    {
        if (probe_recs.empty()) return 0;
        for (uint32_t i : probe_at[point][after]) {
            const ProbeRec &p = probe_recs[i];
            if (p.r.section == ZKGPU_PROBE_SCALARS) {
                memcpy(&probe_payload[p.r.vals_off], ch, 24 * 8);
                if (!evals.empty()) memcpy(&probe_payload[p.r.vals_off + 24], evals.data(), evals.size() * 8);
                continue;
            }
            CK(zkgpu_gather_rows_dev(probe_stage + p.stage, S.sec[p.r.section], S.ld[p.r.section], p.r.ncols,
                                     probe_rows + p.rows_dev, p.r.n_rows));
        }
        return 0;
    }
    // after the proof's last kernel and its total timer: the one copy to the host
    int probe_readback()
    {
        if (probe_recs.empty()) return 0;
        const auto t = clk::now();
        CK(zkgpu_memcpy_d2h(probe_payload.data() + probe_gather0, probe_stage, probe_stage_words * 8));
        timers.emplace_back("ZKGPU_PROBE_READBACK", std::chrono::duration<double, std::milli>(clk::now() - t).count());
        probe_valid = true;
        return 0;
    }
    int probe_size(uint32_t *n_recs, uint64_t *n_words) const
    {
        if (n_recs) *n_recs = probe_valid ? (uint32_t)probe_recs.size() : 0;
        if (n_words) *n_words = probe_valid ? probe_payload.size() : 0;
        return 0;
    }
    int probe_read(zkgpu_probe_rec *recs, uint32_t max_recs, uint64_t *payload, uint64_t max_words) const
    {
        if (!probe_valid)
            return fail("probe_read: no probe to read: none was set (probe_set) before the last proof, or that proof "
                        "failed");
        if (!recs || !payload) return fail("probe_read: null buffer");
        if (max_recs < probe_recs.size() || max_words < probe_payload.size())
            return fail("probe_read: buffers of %u records / %llu words are too small for %zu records / %zu words "
                        "(probe_size)", max_recs, (unsigned long long)max_words, probe_recs.size(),
                        probe_payload.size());
        for (size_t i = 0; i < probe_recs.size(); i++) recs[i] = probe_recs[i].r;
        memcpy(payload, probe_payload.data(), probe_payload.size() * 8);
        return 0;
    }

    // ---- constraint check (include/zkgpu_stark.h zkgpu_stark_check_*): the
    // quotient program on the trace domain, before stage 3's commit.  The
    // combination C that step42ns forms before its "x ZI" is zero on every
    // row of <omega_n> iff the trace satisfies every identity, so the same
    // instruction list over the n-domain sections (check_opnd: step42ns's
    // operands rewritten by zkgpu_zxp_to_n_domain) names the rows that break
    // the AIR at 1 / 2^blowup of the quotient's rows.  Its 3 output columns
    // borrow the head of q (dead until stage 4); the rows that are not zero
    // come from zkgpu_nonzero_rows_dev into a 20-word device block of the
    // check's own (outside the memory plan, as the probe's).
    uint32_t check_mode = ZKGPU_CHECK_OFF;
    std::vector<zxp_operand> check_opnd;
    uint64_t *check_dev = nullptr;  // [0] n_bad, [1, 17) rows, [17, 20) C at the first
    bool check_pending = false;     // REPORT: the block is read back after the proof
    zkgpu_check_result check_res = {};

    virtual int check_set(uint32_t mode)
    {
        if (mode > ZKGPU_CHECK_STOP) return fail("check_set: unknown mode %u", mode);
        if (mode == ZKGPU_CHECK_OFF) {
            check_mode = ZKGPU_CHECK_OFF;
            return 0;
        }
        std::string why;
        if (!check_prepare(why)) {
            check_mode = ZKGPU_CHECK_OFF;
            return fail("check_set: %s; the check is off", why.c_str());
        }
        check_mode = mode;
        return 0;
    }
    // the n-domain rewrite of step42ns (once) and the check's device block; false: `why` says what
    // was refused (the mode is the caller's business: the audit uses the check without setting one)
    bool check_prepare(std::string &why)
    {
        if (check_opnd.empty()) {
            std::vector<zxp_operand> o(step42ns.opnd.size() + 1);
            if (zkgpu_zxp_to_n_domain(o.data(), step42ns.instr.data(), (uint32_t)step42ns.instr.size(),
                                      step42ns.opnd.data(), (uint32_t)step42ns.opnd.size(), eb)) {
                why = std::string("step42ns: ") + zkgpu_last_error();
                return false;
            }
            o.resize(step42ns.opnd.size());
            check_opnd.swap(o);
        }
        if (!check_dev) {
            void *v = nullptr;
            if (zkgpu_dev_malloc(&v, (4 + ZKGPU_CHECK_MAX_ROWS) * 8)) {
                why = zkgpu_last_error();
                return false;
            }
            check_dev = (uint64_t *)v;
        }
        return true;
    }

    // between the last stage-3 program and stage 3's commit: every n-domain
    // section is alive under both memory plans.  The combination challenge
    // (challenge 4) comes from root 3, which does not exist yet, so the check
    // takes its own: the getField of a COPY of the transcript as it stands
    // (challenges 2 and 3 drawn); the proof's transcript is not touched.
    int check_run(const Transcript &tr, const uint64_t ch[24])
    {
        if (check_queue(tr, ch, "ZKGPU_CHECK_CONSTRAINTS")) return -1;
        if (check_mode == ZKGPU_CHECK_REPORT) {
            check_pending = true;
            return 0;
        }
        if (check_readback()) return -1;  // STOP: the one synchronisation
        if (check_res.n_bad) {
            // the terms that fail at the first row, up to 8 (with naming on)
            std::string tail;
            if (names_on) {
                const std::vector<uint32_t> &ids = names_ids[0];
                if (!ids.empty()) tail = "; failing terms there:";
                for (size_t k = 0; k < ids.size() && k < 8; k++) tail += " " + std::to_string(ids[k]);
                if (ids.size() > 8) tail += " and " + std::to_string(ids.size() - 8) + " more";
                if (!ids.empty()) tail += " (zkgpu_stark_check_named)";
            }
            return fail("constraint check: %llu of the 2^%u = %llu rows of the trace break the AIR; the first is row "
                        "%llu (zkgpu_stark_check_result lists the lowest %u)%s",
                        (unsigned long long)check_res.n_bad, info.n_bits, (unsigned long long)N,
                        (unsigned long long)check_res.rows[0], (unsigned)ZKGPU_CHECK_MAX_ROWS, tail.c_str());
        }
        return 0;
    }
    // the check's launches (and, with naming on, the names') under one timer line; nothing is read back
    int check_queue(const Transcript &tr, const uint64_t ch[24], const char *timer)
    {
        tstart();
        Transcript fork = tr;
        uint64_t chk[24];
        memcpy(chk, ch, sizeof chk);
        fork.get_field(chk + 12);
        memcpy(check_res.alpha, chk + 12, 24);
        zkgpu_sections T = S;
        const uint32_t pairs[4][2] = {{SEC_CM1_2NS, SEC_CM1_N}, {SEC_CM2_2NS, SEC_CM2_N}, {SEC_CM3_2NS, SEC_CM3_N},
                                      {SEC_CONST_2NS, SEC_CONST_N}};
        for (const auto &p : pairs) {
            T.sec[p[0]] = S.sec[p[1]];
            T.ld[p[0]] = N;
            T.ncols[p[0]] = S.ncols[p[1]];
        }
        uint64_t *c = S.sec[SEC_Q_2NS];  // its first 3 N words, ld N
        T.ld[SEC_Q_2NS] = N;
        const uint64_t ev0[3] = {0, 0, 0};
        CK(zkgpu_zxp_eval_dev(step42ns.instr.data(), (uint32_t)step42ns.instr.size(), check_opnd.data(),
                              (uint32_t)check_opnd.size(), step42ns.n_tmp1 ? step42ns.n_tmp1 : 1,
                              step42ns.n_tmp3 ? step42ns.n_tmp3 : 1, &T, info.n_bits, chk, publics.data(),
                              (uint32_t)publics.size(), ev0, 0, nullptr, nullptr, 0, 1));
        CK(zkgpu_nonzero_rows_dev(check_dev, c, N, 3, N, ZKGPU_CHECK_MAX_ROWS));
        // C at the first failing row (a row index past the domain -- none failed -- reads 0)
        CK(zkgpu_gather_rows_dev(check_dev + 1 + ZKGPU_CHECK_MAX_ROWS, c, N, 3, check_dev + 1, 1));
        if (names_on) {
            // every term of C at the listed rows: the tapped program over the same sections, its
            // 3K output columns the names' block (ld 16), the row list the check's own on the device
            T.sec[SEC_Q_2NS] = names_dev;
            T.ld[SEC_Q_2NS] = ZKGPU_CHECK_MAX_ROWS;
            T.ncols[SEC_Q_2NS] = 3 * (uint32_t)names_terms.size();
            CK(zkgpu_zxp_eval_rows_dev(names_instr.data(), (uint32_t)names_instr.size(), names_opnd.data(),
                                       (uint32_t)names_opnd.size(), step42ns.n_tmp1 ? step42ns.n_tmp1 : 1,
                                       step42ns.n_tmp3 ? step42ns.n_tmp3 : 1, &T, info.n_bits, chk, publics.data(),
                                       (uint32_t)publics.size(), ev0, 0, nullptr, nullptr, 0, 1, check_dev + 1,
                                       ZKGPU_CHECK_MAX_ROWS));
        }
        return tstop(timer);
    }
    int check_readback()
    {
        uint64_t h[4 + ZKGPU_CHECK_MAX_ROWS];
        CK(zkgpu_memcpy_d2h(h, check_dev, sizeof h));
        check_res.n_bad = h[0];
        memcpy(check_res.rows, h + 1, ZKGPU_CHECK_MAX_ROWS * 8);
        for (int k = 0; k < 3; k++) check_res.value[k] = h[1 + ZKGPU_CHECK_MAX_ROWS + k] % P;
        check_res.ran = 1;
        check_pending = false;
        for (auto &v : names_ids) v.clear();
        for (auto &v : names_vals) v.clear();
        names_ran = names_on;
        if (names_on && check_res.n_bad) {
            // the names' block: only with a failing row, only its first min(n_bad, 16) rows count
            const size_t K = names_terms.size();
            std::vector<uint64_t> b(3 * K * ZKGPU_CHECK_MAX_ROWS);
            CK(zkgpu_memcpy_d2h(b.data(), names_dev, b.size() * 8));
            const uint64_t n_listed = std::min<uint64_t>(check_res.n_bad, ZKGPU_CHECK_MAX_ROWS);
            for (uint64_t j = 0; j < n_listed; j++)
                for (size_t k = 0; k < K; k++) {
                    if (names_terms[k].dead) continue;
                    uint64_t v[3];
                    for (int t = 0; t < 3; t++) v[t] = b[(3 * k + t) * ZKGPU_CHECK_MAX_ROWS + j] % P;
                    if (!(v[0] | v[1] | v[2])) continue;
                    names_ids[j].push_back((uint32_t)k);
                    names_vals[j].insert(names_vals[j].end(), v, v + 3);
                }
        }
        return 0;
    }

    // ---- naming (zkgpu_stark_check_names_set): which terms of C fail at the listed rows.
    // zkgpu_zxp_split_constraints takes the n-domain step42ns apart once; the tapped program runs
    // at the check's row list (zkgpu_zxp_eval_rows_dev) into a device block of 3K x 16 words of
    // the names' own, outside the memory plan like the check's block.
    bool names_on = false, names_ran = false;
    std::vector<zxp_instr> names_instr;
    std::vector<zxp_operand> names_opnd;
    std::vector<zxp_split_term> names_terms;
    uint64_t *names_dev = nullptr;
    std::vector<uint32_t> names_ids[ZKGPU_CHECK_MAX_ROWS];
    std::vector<uint64_t> names_vals[ZKGPU_CHECK_MAX_ROWS];

    virtual int check_names_set(int on)
    {
        if (!on) {
            names_on = false;
            return 0;
        }
        std::string why;
        if (!names_prepare(why)) {
            names_on = false;
            return fail("check_names_set: %s; naming is off", why.c_str());
        }
        names_on = true;
        return 0;
    }
    // the split of the n-domain step42ns (once) and the names' device block; false: `why` says
    // what was refused (whether naming is on is the caller's business, as with check_prepare)
    bool names_prepare(std::string &why)
    {
        if (names_terms.empty()) {
            std::vector<zxp_operand> nd(step42ns.opnd.size() + 1);
            if (zkgpu_zxp_to_n_domain(nd.data(), step42ns.instr.data(), (uint32_t)step42ns.instr.size(),
                                      step42ns.opnd.data(), (uint32_t)step42ns.opnd.size(), eb)) {
                why = std::string("step42ns: ") + zkgpu_last_error();
                return false;
            }
            const size_t ni = step42ns.instr.size(), no = step42ns.opnd.size();
            std::vector<zxp_instr> ti(2 * ni + 1);
            std::vector<zxp_operand> to(no + 2 * ni + 1);
            std::vector<zxp_split_term> tt(2 * ni + 1);
            uint32_t n_i = 0, n_o = 0, n_t = 0;
            if (zkgpu_zxp_split_constraints(ti.data(), &n_i, to.data(), &n_o, tt.data(), &n_t, step42ns.instr.data(),
                                            (uint32_t)ni, nd.data(), (uint32_t)no, 4)) {
                why = std::string("step42ns: ") + zkgpu_last_error();
                return false;
            }
            ti.resize(n_i), to.resize(n_o), tt.resize(n_t);
            names_instr.swap(ti), names_opnd.swap(to), names_terms.swap(tt);
        }
        if (!names_dev) {
            void *v = nullptr;
            if (zkgpu_dev_malloc(&v, 3 * names_terms.size() * ZKGPU_CHECK_MAX_ROWS * 8)) {
                why = zkgpu_last_error();
                return false;
            }
            names_dev = (uint64_t *)v;
        }
        return true;
    }
    int check_terms(zxp_split_term *out, uint32_t max, uint32_t *n) const
    {
        if (!n) return fail("check_terms: null count");
        *n = (uint32_t)names_terms.size();
        if (names_terms.empty()) return fail("check_terms: naming has not been set on this prover");
        if (max && !out) return fail("check_terms: null buffer");
        for (uint32_t k = 0; k < max && k < names_terms.size(); k++) out[k] = names_terms[k];
        return 0;
    }
    int check_named(uint32_t slot, uint32_t *ids, uint64_t *values, uint32_t max, uint32_t *n_failing) const
    {
        if (!n_failing) return fail("check_named: null count");
        *n_failing = 0;
        if (slot >= ZKGPU_CHECK_MAX_ROWS) return fail("check_named: slot %u of %u", slot, (unsigned)ZKGPU_CHECK_MAX_ROWS);
        if (!check_res.ran || !names_ran) return fail("check_named: the last proof ran no check with naming on");
        if (max && (!ids || !values)) return fail("check_named: null buffer");
        const std::vector<uint32_t> &v = names_ids[slot];
        *n_failing = (uint32_t)v.size();
        for (uint32_t k = 0; k < max && k < v.size(); k++) {
            ids[k] = v[k];
            memcpy(values + 3 * k, names_vals[slot].data() + 3 * k, 24);
        }
        return 0;
    }
    int check_result(zkgpu_check_result *out) const
    {
        if (!out) return fail("check_result: null buffer");
        *out = check_res;
        return 0;
    }

    // ---- the steps of prove_body that the row-sharded prover overrides
    // (with quotient_pieces, h1h2_all, z_all, ncol, r0 and the FRI steps)

    // The commit of stage t.  t = 1, 2, 3: extendPol of the stage's n-domain
    // section into its extended one (stage 1 of a streamed or a lean proof in
    // its own way) -- in place (lean plan: the n-domain values sit at the
    // start of the extended region) when the two pointers are equal --, then
    // its tree and root; t = 4, the quotient pieces: tree and root.
    virtual int commit_stage(int t, uint64_t root[4])
    {
        if (t == 1 && stream_rows) return commit_cm1_stream(root);
        if (t == 1 && lean()) return commit_cm1_lean(root);
        const uint32_t sec_e = SEC_CM1_2NS + t - 1, ncols = stage_cols(t);
        if (t < 4) {
            const uint32_t sec_n = SEC_CM1_N + t - 1;
            tstart();
            if (S.sec[sec_e] == S.sec[sec_n])
                CK(zkgpu_gl_extend_pol_inplace_dev(S.sec[sec_e], NE, N, ncols));
            else
                CK(zkgpu_gl_extend_pol_dev(S.sec[sec_e], NE, S.sec[sec_n], N, NE, N, ncols));
            if (tstop_commit(t, "LDE")) return -1;
        }
        tstart();
        CK(zkgpu_gl_merkletree_dev(nodes[t - 1], S.sec[sec_e], NE, ncols, NE));
        CK(zkgpu_memcpy_d2h(root, nodes[t - 1] + zkgpu_gl_merkle_num_elements(NE) - 4, 32));
        return tstop_commit(t, "MERKLETREE");
    }
    // The stage program p of probe point `point`: ZKGPU_PROBE_STEP2 /
    // STEP3PREV / STEP3 on the n domain, STEP42NS / STEP52NS on the extended
    // one (the last reads the evaluations); here between its two probe points.
    virtual int run_prog(uint32_t point, const Prog &p, const uint64_t ch[24], const std::vector<uint64_t> &evals)
    {
        const bool ext = point == ZKGPU_PROBE_STEP42NS || point == ZKGPU_PROBE_STEP52NS;
        const uint32_t n_ev = point == ZKGPU_PROBE_STEP52NS ? info.n_ev : 0;
        if (probe_point(point, 0, ch, evals) || run(p, ext, ch, evals.data(), n_ev)) return -1;
        return probe_point(point, 1, ch, evals);
    }
    // evmap's sums over rows [r0(), r0() + nb) -> the evaluations (all rows: they are)
    virtual int sum_evals(std::vector<uint64_t> &) { return 0; }
    virtual int xdivxsub(const uint64_t xi[3])
    {
        CK(zkgpu_xdivxsub_dev(xdiv, xdivw, xi, info.n_bits, info.n_bits_ext));
        return 0;
    }
    // the FRI polynomial (SEC_F_2NS, 3 columns) interleaved into fri_pol[0]
    virtual int fill_fri_pol0()
    {
        CK(zkgpu_cols3_to_interleaved_dev(fri_pol[0], S.sec[SEC_F_2NS], NE, NE));
        return 0;
    }

    // The one Fiat-Shamir schedule of the single-GPU and the row-sharded
    // prover: the order of the transcript's inputs and challenges, the stage
    // boundaries and the stage timers (the FRI part: fri_and_queries).  The
    // row-sharded prover is never lean (shape() leaves mem_mode RESIDENT) and
    // refuses probe_set and prove_from_rows: the lean(), probe_recs and
    // stream_rows branches are dead there.
    int prove_body(uint64_t *out)
    {
        probe_valid = false;
        check_pending = false;
        check_res = zkgpu_check_result{};
        zdiag = zkgpu_z_diag{};
        names_ran = false;
        for (auto &v : names_ids) v.clear();
        for (auto &v : names_vals) v.clear();
        timers.clear();
        pend_t.clear();
        pend_x.clear();
        n_marks = 0;
        auto tall = clk::now();
        Transcript tr;
        tr.put(verkey, 4);
        tr.put(publics.data(), publics.size());
        uint64_t ch[24] = {0};
        uint64_t roots[4][4];
        std::vector<uint64_t> evals(3 * info.n_ev);
        auto commit_root = [&](int t) {  // stage t's commit, its root into the transcript
            if (commit_stage(t, roots[t - 1])) return -1;
            tr.put(roots[t - 1], 4);
            return 0;
        };
        // STAGE 1 (starks.cpp:49-63)
        if (commit_root(1)) return -1;
        // lean: the regions of tmpExp_n / cm2_n / cm3_n held other sections;
        // the columns no stage writes read 0, as under the resident plan
        if (lean() && (zero_unwritten(SEC_TMP_N) || zero_unwritten(SEC_CM2_N) || zero_unwritten(SEC_CM3_N)))
            return -1;
        // probed: a column no stage of this proof has written yet reads 0 in a
        // record, as in a fresh prover (and the CPU provers' zeroed memory),
        // not the last proof's values or, lean, those of the region's former
        // section (the regions are dead here, as for zero_unwritten)
        if (!probe_recs.empty())
            for (uint32_t s : {SEC_TMP_N, SEC_CM2_N, SEC_CM3_N})
                CK(zkgpu_memset_dev(S.sec[s], 0, (uint64_t)S.ncols[s] * N * 8));
        // STAGE 2 (:65-144)
        tr.get_field(ch + 0);
        tr.get_field(ch + 3);
        tstart();
        if (run_prog(ZKGPU_PROBE_STEP2, step2, ch, evals)) return -1;
        if (tstop("STARK_STEP_2_CALCULATE_EXPS")) return -1;
        if (info.n_pu) {
            tstart();
            if (probe_point(ZKGPU_PROBE_H1H2, 0, ch, evals) || h1h2_all() ||
                probe_point(ZKGPU_PROBE_H1H2, 1, ch, evals))
                return -1;
            if (tstop("STARK_STEP_2_CALCULATEH1H2")) return -1;
        }
        if (commit_root(2)) return -1;
        // STAGE 3 (:146-224)
        tr.get_field(ch + 6);
        tr.get_field(ch + 9);
        tstart();
        if (run_prog(ZKGPU_PROBE_STEP3PREV, step3prev, ch, evals)) return -1;
        if (tstop("STARK_STEP_3_CALCULATE_EXPS")) return -1;
        tstart();
        if (probe_point(ZKGPU_PROBE_Z, 0, ch, evals) || z_all() || probe_point(ZKGPU_PROBE_Z, 1, ch, evals)) return -1;
        if (tstop("STARK_STEP_3_CALCULATE_Z")) return -1;
        // step3: post-Z expressions (starks.cpp:193-208)
        if (!step3.instr.empty()) {
            tstart();
            if (run_prog(ZKGPU_PROBE_STEP3, step3, ch, evals)) return -1;
            if (tstop("STARK_STEP_3_CALCULATE_EXPS_2")) return -1;
        }
        if (check_mode != ZKGPU_CHECK_OFF && check_run(tr, ch)) return -1;
        if (commit_root(3)) return -1;
        // STAGE 4 (:226-296)
        tr.get_field(ch + 12);
        if (lean()) {
            // cm1_2ns again, over cm1_n (tmpExp_n / cm2_n above it are dead):
            // the columns not kept extended in place, the kept ones copied
            tstart();
            cm1_consumed = true;
            const uint64_t split = info.n_cm1 - keep_cols;
            if (split) CK(zkgpu_gl_extend_pol_inplace_dev(arena, NE, N, split));
            if (keep_cols) CK(zkgpu_memcpy_d2d(arena + split * NE, keep, keep_cols * NE * 8));
            S.sec[SEC_CM1_2NS] = arena;
            if (tstop("STARK_STEP_4_CM1_LDE")) return -1;
        }
        tstart();
        if (run_prog(ZKGPU_PROBE_STEP42NS, step42ns, ch, evals)) return -1;
        if (tstop("STARK_STEP_4_CALCULATE_EXPS_2NS")) return -1;
        tstart();
        if (probe_point(ZKGPU_PROBE_QSPLIT, 0, ch, evals) || quotient_pieces() ||
            probe_point(ZKGPU_PROBE_QSPLIT, 1, ch, evals))
            return -1;
        if (tstop("STARK_STEP_4_CALCULATE_EXPS_2NS_INTT_NTT")) return -1;
        if (commit_root(4)) return -1;
        // STAGE 5 (:298-392)
        tstart();
        uint64_t *xi = ch + 21;
        tr.get_field(xi);
        // Starks::evmap (starks.cpp:308-333,556-669) interpolates every
        // polynomial from its extension rows k << eb, the coset points
        // 7 w_N^k, with L = INTT((xi/7)^i).  The same values pol(xi) come
        // from the n-domain rows (points w_N^k) with L = INTT(xi^i): the
        // polynomial of degree < N is the same, the field sums are exact, and
        // contiguous n-domain columns read half the lines of the strided
        // extension rows.
        if (lean()) {
            // the extended rows k << eb are the points 7 w_N^k: the weights of
            // xi / 7 (starks.cpp:316-322)
            const uint64_t i7 = inv(7), xs[3] = {mul(xi[0], i7), mul(xi[1], i7), mul(xi[2], i7)};
            if (lagrange_xi(xs, r0(), nb)) return -1;
        } else if (lagrange_xi(xi, r0(), nb)) {
            return -1;
        }
        if (tstop("STARK_STEP_5_LEv_LpEv")) return -1;
        tstart();
        if (evmap_rows(r0(), nb, evals.data()) || sum_evals(evals)) return -1;
        if (tstop("STARK_STEP_5_EVMAP")) return -1;
        tr.put(evals.data(), evals.size());
        tr.get_field(ch + 15);
        tr.get_field(ch + 18);
        tstart();
        if (xdivxsub(xi)) return -1;
        if (tstop("STARK_STEP_5_XDIVXSUB")) return -1;
        tstart();
        if (run_prog(ZKGPU_PROBE_STEP52NS, step52ns, ch, evals) || fill_fri_pol0()) return -1;
        if (tstop("STARK_STEP_5_CALCULATE_EXPS")) return -1;
        if (fri_and_queries(tr, &roots[0][0], evals, out, tall)) return -1;
        if (check_pending && check_readback()) return -1;
        return probe_readback();
    }

    // calculateH1H2 of every plookup (starks.cpp:104-127), n domain
    virtual int h1h2_all()
    {
        for (uint32_t k = 0; k < info.n_pu; k++) {
            const uint32_t *q = &pu[5 * k];
            uint64_t miss = 0;
            const int rc = zkgpu_h1h2_dev(S.sec[SEC_CM2_N] + (uint64_t)q[2] * N, N,
                                          S.sec[SEC_CM2_N] + (uint64_t)q[3] * N, N,
                                          S.sec[SEC_TMP_N] + (uint64_t)q[0] * N, N,
                                          S.sec[SEC_TMP_N] + (uint64_t)q[1] * N, N, N, q[4], &miss);
            if (rc) {
                if (miss != ~0ULL)
                    return fail("Polinomial::calculateH1H2() Number not included: w=%llu plookup_number=%u",
                                (unsigned long long)miss, k);
                return fail("calculateH1H2: %s", zkgpu_last_error());
            }
        }
        return 0;
    }

    // calculateZ of every grand product (starks.cpp:165-189), n domain
    std::vector<zkgpu_z_req> z_requests() const
    {
        std::vector<zkgpu_z_req> req(info.n_zctx);
        for (uint32_t z = 0; z < info.n_zctx; z++)
            req[z] = {S.sec[SEC_CM3_N] + (uint64_t)zctx[3 * z + 2] * N, N, S.sec[SEC_TMP_N] + (uint64_t)zctx[3 * z] * N, N,
                      S.sec[SEC_TMP_N] + (uint64_t)zctx[3 * z + 1] * N, N};
        return req;
    }
    virtual int z_all()
    {
        const std::vector<zkgpu_z_req> req = z_requests();
        std::vector<int> closes(info.n_zctx + 1, 0);
        CK(zkgpu_calculate_z_many_dev(req.data(), info.n_zctx, N, closes.data()));
        uint32_t n_open = 0, first = 0;
        for (uint32_t z = info.n_zctx; z-- > 0;)
            if (!closes[z]) n_open++, first = z;
        return n_open ? z_open(first, n_open) : 0;
    }

    // ---- a grand product that does not close: which values keep it open
    // The failing path of z_all (a proof whose products close queues nothing
    // of this): the multiset comparison (zkgpu_multiset_diff_dev) of the num
    // and den tmpExp columns of the lowest open product, read back into
    // zdiag before the failure returns.  For a permutation check (num = f +
    // gamma, den = t + gamma) the lists are the offending values and where
    // they first occur; the per-row factors of a plookup or connection
    // product are not paired values: those faults are named by the audit's
    // lookup misses and by conn_check / audit_conn below.  The 98-word result block lives for this call only.
    zkgpu_z_diag zdiag = {};

    int z_open(uint32_t z, uint32_t n_open)
    {
        zdiag = zkgpu_z_diag{};
        zdiag.z = z;
        zdiag.n_open = n_open;
        std::string why;
        if (!z_compare(z, zdiag.n_num, zdiag.n_den, zdiag.num, zdiag.den, why))
            return fail("calculateZ: grand product %u does not close (%u of %u do not); the comparison of its num and "
                        "den columns was skipped: %s", z, n_open, info.n_zctx, why.c_str());
        zdiag.ran = 1;
        char side[2][160];
        for (int b = 0; b < 2; b++) {
            const uint64_t cnt = b ? zdiag.n_den : zdiag.n_num;
            const zkgpu_z_diag_val &v = b ? zdiag.den[0] : zdiag.num[0];
            const char *name = b ? "den" : "num";
            if (cnt)
                snprintf(side[b], sizeof side[b], "%llu value(s) of %s unmatched, the first at row %llu (%llu in num, "
                         "%llu in den)", (unsigned long long)cnt, name, (unsigned long long)v.row,
                         (unsigned long long)v.count_num, (unsigned long long)v.count_den);
            else
                snprintf(side[b], sizeof side[b], "no value of %s unmatched", name);
        }
        return fail("calculateZ: grand product %u does not close (%u of %u do not): %s; %s", z, n_open, info.n_zctx,
                    side[0], side[1]);
    }

    // the num and den columns of product z compared as multisets into the lists of zkgpu_z_diag (the
    // audit's too); false: the scratch or the result block could not be had, `why` says which
    bool z_compare(uint32_t z, uint64_t &n_num, uint64_t &n_den, zkgpu_z_diag_val *num, zkgpu_z_diag_val *den,
                   std::string &why)
    {
        constexpr uint32_t M = ZKGPU_Z_DIAG_MAX, BLK = 1 + 3 * M;
        uint64_t h[2 * BLK];
        void *dev = nullptr;
        int rc = zkgpu_dev_malloc(&dev, sizeof h);
        if (!rc)
            rc = zkgpu_multiset_diff_dev((uint64_t *)dev, S.sec[SEC_TMP_N] + (uint64_t)zctx[3 * z] * N, N,
                                         S.sec[SEC_TMP_N] + (uint64_t)zctx[3 * z + 1] * N, N, N, 3, M);
        if (!rc) rc = zkgpu_memcpy_d2h(h, dev, sizeof h);
        why = rc ? zkgpu_last_error() : "";
        (void)zkgpu_dev_free(dev);
        if (rc) return false;
        n_num = h[0];
        n_den = h[BLK];
        for (uint32_t k = 0; k < M; k++) {
            num[k] = {h[1 + 3 * k], h[2 + 3 * k], h[3 + 3 * k]};
            den[k] = {h[BLK + 1 + 3 * k], h[BLK + 2 + 3 * k], h[BLK + 3 + 3 * k]};
        }
        return true;
    }

    virtual int z_diag(zkgpu_z_diag *out) const
    {
        if (!out) return fail("z_diag: null buffer");
        *out = zdiag;
        return 0;
    }

    // ---- trace audit (include/zkgpu_stark.h zkgpu_stark_audit): the stage-2
    // and stage-3 work of prove_body on the n domain, run to the end whatever
    // it finds, with challenges from a transcript that holds no root.  It
    // writes tmpExp_n, cm2_n, cm3_n and the head of q -- every one dead between
    // proofs under both plans -- and reads cm1_n, which it leaves as it is.
    // The programs go through run(), not run_prog(): no probe record is taken.
    zkgpu_audit_report audit_rep = {};
    bool audit_valid = false, audit_named = false;
    std::string audit_why;  // why the identities did not run although no plookup missed
    std::vector<std::vector<uint32_t>> audit_terms;  // with naming: the failing term ids per listed row

    // layer A's finding: the f values of plookup k that its table does not hold (a 34-word result
    // block that lives for this call, as z_compare's)
    int audit_misses(uint32_t k, zkgpu_audit_pu &e)
    {
        constexpr uint32_t M = ZKGPU_LOOKUP_MISS_MAX;
        const uint32_t *q = &pu[5 * k];
        uint64_t h[2 + 2 * M];
        void *dev = nullptr;
        int rc = zkgpu_dev_malloc(&dev, sizeof h);
        if (!rc)
            rc = zkgpu_lookup_misses_dev((uint64_t *)dev, S.sec[SEC_TMP_N] + (uint64_t)q[0] * N, N,
                                         S.sec[SEC_TMP_N] + (uint64_t)q[1] * N, N, N, q[4], M);
        if (!rc) rc = zkgpu_memcpy_d2h(h, dev, sizeof h);
        const std::string why = rc ? zkgpu_last_error() : "";
        (void)zkgpu_dev_free(dev);
        if (rc) return fail("audit: plookup %u: %s", k, why.c_str());
        e.pu = k;
        e.n_rows = h[0];
        e.n_vals = h[1];
        for (uint32_t j = 0; j < M; j++) e.vals[j] = {h[2 + 2 * j], h[3 + 2 * j]};
        return 0;
    }

    // ---- connection checks (include/zkgpu_stark.h zkgpu_stark_conn_set): product z of zctx declared as
    // {cm1 columns} connect {constant columns}; conn_run names the cells that keep it open
    // (zkgpu_conn_breaks_dev over cm1_n and const_n, one synchronisation, a 99-word result block
    // that lives for the call).  Neither section is written.
    struct ConnDecl {
        std::vector<uint32_t> cm1_cols, const_cols;
        std::vector<uint64_t> ks;  // empty: the default shifts
    };
    std::map<uint32_t, ConnDecl> conns;
    zkgpu_conn_report audit_conns[ZKGPU_AUDIT_MAX_Z] = {};  // by index into audit_rep.z

    virtual int conn_set(uint32_t z, const zkgpu_conn_desc *d)
    {
        if (z >= info.n_zctx) return fail("conn_set: product %u: the instance has %u grand product(s)", z, info.n_zctx);
        if (!d) {
            conns.erase(z);
            return 0;
        }
        if (!d->cm1_cols || !d->const_cols) return fail("conn_set: product %u: null column list", z);
        if (zkgpu_conn_ks_check(d->ks, d->k, info.n_bits)) return fail("conn_set: product %u: %s", z, zkgpu_last_error());
        ConnDecl c;
        for (uint32_t i = 0; i < d->k; i++) {
            if (d->cm1_cols[i] >= info.n_cm1)
                return fail("conn_set: product %u: cm1 column %u: the instance has %u", z, d->cm1_cols[i], info.n_cm1);
            if (d->const_cols[i] >= info.n_const)
                return fail("conn_set: product %u: constant column %u: the instance has %u", z, d->const_cols[i],
                            info.n_const);
            for (uint32_t j = 0; j < i; j++)
                if (d->cm1_cols[j] == d->cm1_cols[i] || d->const_cols[j] == d->const_cols[i])
                    return fail("conn_set: product %u: column %u repeated", z,
                                d->cm1_cols[j] == d->cm1_cols[i] ? d->cm1_cols[i] : d->const_cols[i]);
        }
        c.cm1_cols.assign(d->cm1_cols, d->cm1_cols + d->k);
        c.const_cols.assign(d->const_cols, d->const_cols + d->k);
        if (d->ks) c.ks.assign(d->ks, d->ks + d->k);
        conns[z] = std::move(c);
        return 0;
    }

    int conn_run(uint32_t z, const ConnDecl &c, zkgpu_conn_report &r, std::string &why)
    {
        constexpr uint32_t M = ZKGPU_CONN_MAX;
        uint64_t h[3 + 6 * M];
        void *dev = nullptr;
        const uint32_t k = (uint32_t)c.cm1_cols.size();
        int rc = zkgpu_dev_malloc(&dev, sizeof h);
        if (!rc)
            rc = zkgpu_conn_breaks_dev((uint64_t *)dev, S.sec[SEC_CM1_N], N, c.cm1_cols.data(), S.sec[SEC_CONST_N], N,
                                       c.const_cols.data(), k, c.ks.empty() ? nullptr : c.ks.data(), info.n_bits, M);
        if (!rc) rc = zkgpu_memcpy_d2h(h, dev, sizeof h);
        why = rc ? zkgpu_last_error() : "";
        (void)zkgpu_dev_free(dev);
        if (rc) return rc;
        r = zkgpu_conn_report{};
        r.ran = 1;
        r.z = z;
        r.n_broken = h[0], r.n_foreign = h[1], r.n_untargeted = h[2];
        for (uint32_t e = 0; e < M; e++) {
            const uint64_t *b = h + 3 + 4 * e, *f = h + 3 + 4 * M + 2 * e;
            zkgpu_conn_break &o = r.breaks[e];
            if (b[0] == UINT64_MAX)
                o = {UINT32_MAX, 0, UINT64_MAX, 0, 0, 0};
            else
                o = {(uint32_t)(b[0] >> info.n_bits), (uint32_t)(b[1] >> info.n_bits), b[0] & (N - 1), b[1] & (N - 1),
                     b[2], b[3]};
            if (f[0] == UINT64_MAX)
                r.foreign[e] = {UINT32_MAX, UINT64_MAX, 0};
            else
                r.foreign[e] = {(uint32_t)(f[0] >> info.n_bits), f[0] & (N - 1), f[1]};
        }
        return 0;
    }

    // the audit's preconditions, in its words
    int need_trace(const char *who)
    {
        if (cm1_broken)
            return fail("%s: the last streamed load (prove_from_rows) failed part-way: no whole trace is loaded; "
                        "load one with set_cm1 or witness first", who);
        if (lean() && cm1_consumed)
            return fail("%s: the previous proof consumed the trace (lean memory plan: cm1_n is extended in place); "
                        "load the next one with set_cm1 or witness first", who);
        if (!cm1_loaded) return fail("%s: no trace is loaded; load one with set_cm1 or witness first", who);
        return 0;
    }

    virtual int conn_check(uint32_t z, zkgpu_conn_report *out)
    {
        if (!out) return fail("conn_check: null buffer");
        if (z >= info.n_zctx)
            return fail("conn_check: product %u: the instance has %u grand product(s)", z, info.n_zctx);
        const auto it = conns.find(z);
        if (it == conns.end()) return fail("conn_check: product %u is not declared a connection (conn_set)", z);
        if (need_trace("conn_check")) return -1;
        std::string why;
        if (conn_run(z, it->second, *out, why)) return fail("conn_check: product %u: %s", z, why.c_str());
        return 0;
    }

    virtual int audit_conn(uint32_t k, zkgpu_conn_report *out) const
    {
        if (!out) return fail("audit_conn: null buffer");
        if (!audit_valid) return fail("audit_conn: no audit has run on this prover");
        if (k >= ZKGPU_AUDIT_MAX_Z) return fail("audit_conn: entry %u: the report lists %u", k, ZKGPU_AUDIT_MAX_Z);
        *out = audit_conns[k];
        return 0;
    }

    virtual int audit(uint32_t flags, zkgpu_audit_report *out)
    {
        if (!out) return fail("audit: null buffer");
        if (flags & ~ZKGPU_AUDIT_NAMES) return fail("audit: unknown flags 0x%x", flags);
        if (need_trace("audit")) return -1;
        audit_valid = false;
        audit_rep = zkgpu_audit_report{};
        for (zkgpu_conn_report &c : audit_conns) c = zkgpu_conn_report{};
        audit_why.clear();
        check_pending = false;
        check_res = zkgpu_check_result{};
        for (uint64_t &row : check_res.rows) row = UINT64_MAX;  // an empty list, should layer C not run
        zdiag = zkgpu_z_diag{};
        names_ran = false;
        for (auto &v : names_ids) v.clear();
        for (auto &v : names_vals) v.clear();
        timers.clear();
        pend_t.clear();
        pend_x.clear();
        n_marks = 0;
        const auto tall = clk::now();
        zkgpu_audit_report &R = audit_rep;
        // the audit's own challenges: verkey and publics, no root
        Transcript tr;
        tr.put(verkey, 4);
        tr.put(publics.data(), publics.size());
        uint64_t ch[24] = {0};
        for (int k = 0; k < 4; k++) tr.get_field(ch + 3 * k);
        {
            Transcript fork = tr;  // (check_queue draws the same value from its own copy)
            uint64_t alpha[3];
            fork.get_field(alpha);
            if (fork.err) return fail("audit: transcript hashing failed: %s", zkgpu_last_error());
            memcpy(R.challenges, ch, 12 * 8);
            memcpy(R.challenges + 12, alpha, 24);
            memcpy(check_res.alpha, alpha, 24);  // (reported whether or not layer C runs)
        }
        const uint64_t ev0[3] = {0, 0, 0};
        // as a proof after stage 1: the columns no stage writes read 0
        if (lean() && (zero_unwritten(SEC_TMP_N) || zero_unwritten(SEC_CM2_N) || zero_unwritten(SEC_CM3_N)))
            return -1;
        // ---- layer A: every plookup
        tstart();
        if (run(step2, false, ch, ev0, 0)) return -1;
        if (tstop("AUDIT_STEP2")) return -1;
        if (info.n_pu) {
            tstart();
            for (uint32_t k = 0; k < info.n_pu; k++) {
                const uint32_t *q = &pu[5 * k];
                uint64_t *h1 = S.sec[SEC_CM2_N] + (uint64_t)q[2] * N, *h2 = S.sec[SEC_CM2_N] + (uint64_t)q[3] * N;
                const uint64_t *f = S.sec[SEC_TMP_N] + (uint64_t)q[0] * N, *t = S.sec[SEC_TMP_N] + (uint64_t)q[1] * N;
                uint64_t miss = ~0ULL;
                const int rc = zkgpu_h1h2_dev(h1, N, h2, N, f, N, t, N, N, q[4], &miss);
                if (!rc) continue;
                if (miss == ~0ULL) return fail("audit: calculateH1H2: %s", zkgpu_last_error());
                // a miss: h1 / h2 were not written; they read zero from here on
                CK(zkgpu_memset_dev(h1, 0, (uint64_t)q[4] * N * 8));
                CK(zkgpu_memset_dev(h2, 0, (uint64_t)q[4] * N * 8));
                if (R.n_pu_bad++ < ZKGPU_AUDIT_MAX_PU && audit_misses(k, R.pu[R.n_pu_bad - 1])) return -1;
            }
            if (tstop("AUDIT_H1H2")) return -1;
        }
        // ---- layer B: every grand product
        tstart();
        if (run(step3prev, false, ch, ev0, 0)) return -1;
        if (tstop("AUDIT_STEP3PREV")) return -1;
        tstart();
        {
            const std::vector<zkgpu_z_req> req = z_requests();
            std::vector<int> closes(info.n_zctx + 1, 0);
            // (every z column is written, closed or not: layer C reads them)
            CK(zkgpu_calculate_z_many_dev(req.data(), info.n_zctx, N, closes.data()));
            for (uint32_t z = 0; z < info.n_zctx; z++) {
                if (closes[z]) continue;
                if (R.n_z_open++ >= ZKGPU_AUDIT_MAX_Z) continue;
                zkgpu_audit_z &e = R.z[R.n_z_open - 1];
                e.z = z;
                // the products one after the other through the shared workspace; without the scratch
                // the product is still listed
                std::string why;
                e.compared = z_compare(z, e.n_num, e.n_den, e.num, e.den, why);
                // a declared connection: the cells that keep it open (ran = 0 without the scratch, as compared)
                const auto it = conns.find(z);
                if (it != conns.end()) (void)conn_run(z, it->second, audit_conns[R.n_z_open - 1], why);
            }
        }
        if (tstop("AUDIT_Z")) return -1;
        if (R.n_z_open) {  // zkgpu_stark_z_diag: the lowest open product
            const zkgpu_audit_z &e = R.z[0];
            zdiag.ran = e.compared;
            zdiag.z = e.z;
            zdiag.n_open = R.n_z_open;
            zdiag.n_num = e.n_num;
            zdiag.n_den = e.n_den;
            memcpy(zdiag.num, e.num, sizeof zdiag.num);
            memcpy(zdiag.den, e.den, sizeof zdiag.den);
        }
        // ---- layer C: the identities, unless a plookup missed (its h1 / h2 read zero)
        audit_named = false;
        audit_terms.clear();
        if (!R.n_pu_bad) {
            if (!step3.instr.empty()) {
                tstart();
                if (run(step3, false, ch, ev0, 0)) return -1;
                if (tstop("AUDIT_STEP3")) return -1;
            }
            if (check_prepare(audit_why)) {
                std::string why_names;
                const bool was_on = names_on;
                names_on = (flags & ZKGPU_AUDIT_NAMES) && names_prepare(why_names);  // refused: rows only
                const int rc = check_queue(tr, ch, "AUDIT_CONSTRAINTS") || check_readback();
                audit_named = names_on;
                if (audit_named) audit_terms.assign(names_ids, names_ids + ZKGPU_CHECK_MAX_ROWS);
                names_on = was_on;
                if (rc) return -1;
            }
        }
        R.identities = check_res;
        R.clean = !R.n_pu_bad && !R.n_z_open && check_res.ran && !check_res.n_bad;
        if (flush_timers()) return -1;
        if (tr.err) return fail("audit: transcript hashing failed: %s", zkgpu_last_error());
        timers.emplace_back("AUDIT_TOTAL", std::chrono::duration<double, std::milli>(clk::now() - tall).count());
        audit_valid = true;
        *out = R;
        return 0;
    }

    virtual int audit_format(char *buf, uint64_t len) const
    {
        if (!audit_valid) return fail("audit_format: no audit has run on this prover");
        if (len && !buf) return fail("audit_format: null buffer");
        AuditContext c;
        c.n_bits = info.n_bits;
        c.n_pu = info.n_pu;
        c.n_zctx = info.n_zctx;
        c.identities_why = audit_why;
        c.named = audit_named;
        c.term_ids = audit_terms;
        c.conn.assign(audit_conns, audit_conns + ZKGPU_AUDIT_MAX_Z);
        const std::string s = zkgpu_host::audit_format(audit_rep, c);
        if (len) {
            const size_t n = std::min<size_t>(s.size(), len - 1);
            memcpy(buf, s.data(), n);
            buf[n] = 0;
        }
        return (int)s.size();
    }

    // LEv / LpEv: the n-domain Lagrange weights of xi and w xi (see prove),
    // rows [row0, row0 + nrows) in closed form (zkgpu_lagrange_xi_rows_dev);
    // the whole domain by interpolation when xi lies in the base field
    int lagrange_xi(const uint64_t xi[3], uint64_t row0, uint64_t nrows)
    {
        if (xi[1] % P || xi[2] % P) {
            CK(zkgpu_lagrange_xi_rows_dev(lev + row0, lpev + row0, N, xi, info.n_bits, row0, nrows));
            return 0;
        }
        uint64_t wN = w_of(info.n_bits);
        uint64_t xis[3], wxis[3];
        for (int k = 0; k < 3; k++) {
            xis[k] = xi[k] % P;
            wxis[k] = mul(xi[k], wN);
        }
        CK(zkgpu_ext_powers_dev(lev, N, xis, N));
        CK(zkgpu_ext_powers_dev(lpev, N, wxis, N));
        CK(zkgpu_gl_ntt_dev(lev, N, lev, N, N, 3, 1));
        CK(zkgpu_gl_ntt_dev(lpev, N, lpev, N, N, 3, 1));
        return 0;
    }

    // starks.cpp:255-296: q (NE x 3, column-major, ld NE) -> INTT -> split
    // into q_deg pieces -> NTT on the coset -> cm4 (n_cm4 x NE); the pieces
    // on the n domain too (cm4_n, for evmap)
    virtual int quotient_pieces()
    {
        CK(zkgpu_gl_ntt_dev(qq1, NE, S.sec[SEC_Q_2NS], NE, NE, 3, 1));
        CK(zkgpu_memset_dev(qq2, 0, (uint64_t)info.n_cm4 * NE * 8));
        uint64_t shift_in = pw(inv(7), N);
        CK(zkgpu_qsplit_dev(qq2, NE, qq1, NE, N, info.q_deg, shift_in));
        CK(zkgpu_gl_ntt_dev(S.sec[SEC_CM4_2NS], NE, qq2, NE, NE, info.n_cm4, 0));
        if (lean()) return 0;  // evmap reads the pieces' extended rows
        // the quotient pieces on the n-domain too (for evmap below): qq2 holds
        // coset-scaled coefficients c_k 7^k (k < N, the rest zero); plain
        // coefficients c_k = qq2_k 7^-k, then NTT_N -> q_p(w_N^j)
        for (uint32_t c = 0; c < info.n_cm4; c++)
            CK(zkgpu_memcpy_d2d(cm4_n + (uint64_t)c * N, qq2 + (uint64_t)c * NE, N * 8));
        CK(zkgpu_scale_by_powers_dev(cm4_n, N, info.n_cm4, N, inv(7)));
        CK(zkgpu_gl_ntt_dev(cm4_n, N, cm4_n, N, N, info.n_cm4, 0));
        return 0;
    }

    // the n-domain values of an evMap entry's polynomial (section_2ns ev_sec,
    // column col) from global row `row` on, and their leading dimension
    virtual const uint64_t *ncol(uint32_t ev_sec, uint32_t col, uint64_t row, uint64_t &ld) const
    {
        ld = N;
        if (ev_sec == SEC_CM4_2NS) return cm4_n + (uint64_t)col * N + row;
        const uint32_t s = ev_sec == SEC_CONST_2NS ? (uint32_t)SEC_CONST_N : ev_sec - SEC_CM1_2NS + SEC_CM1_N;
        return S.sec[s] + (uint64_t)col * N + row;
    }

    // Starks::evmap over n-domain rows [k0, k0 + nrows) (starks.cpp:556-669;
    // the row sum is linear, so row blocks give partial sums)
    int evmap_rows(uint64_t k0, uint64_t nrows, uint64_t *evals_out)
    {
        std::vector<const uint64_t *> cols(info.n_ev);
        std::vector<uint64_t> lds(info.n_ev);
        std::vector<uint32_t> dims(info.n_ev), primes(info.n_ev);
        for (uint32_t e = 0; e < info.n_ev; e++) {
            if (lean()) {  // the extended rows k << eb (the n-domain values are gone)
                lds[e] = NE;
                cols[e] = S.sec[ev[4 * e]] + (uint64_t)ev[4 * e + 1] * NE + (k0 << eb);
            } else {
                cols[e] = ncol(ev[4 * e], ev[4 * e + 1], k0, lds[e]);
            }
            dims[e] = ev[4 * e + 2];
            primes[e] = ev[4 * e + 3];
        }
        CK(zkgpu_evmap_dev(evals_out, cols.data(), lds.data(), dims.data(), primes.data(), info.n_ev, lev + k0,
                           lpev + k0, N, nrows, lean() ? eb : 0));
        return 0;
    }

    // FRIProve::prove + queries (friProve.cpp:5-232) once fri_pol[0] holds the
    // FRI polynomial; s0 openings through open_s0
    int fri_and_queries(Transcript &tr, const uint64_t *roots, const std::vector<uint64_t> &evals, uint64_t *out,
                        clk::time_point tall)
    {
        tstart();
        uint64_t *w = out;
        memcpy(w, roots, 16 * 8);
        w += 16;
        memcpy(w, evals.data(), evals.size() * 8);
        w += evals.size();
        uint32_t pol_bits = info.n_bits_ext;
        uint64_t shift_inv = inv(7);
        int cur = 0;
        std::vector<uint64_t> fri_roots(4 * fri_steps.size(), 0);
        std::vector<uint64_t> final_pol(3ULL << fri_steps.back());
        for (size_t si = 0; si < fri_steps.size(); si++) {
            uint32_t red = pol_bits - fri_steps[si];
            uint64_t sx[3];
            tr.get_field(sx);
            if (si > 0) {
                if (fri_fold_step(si, fri_pol[cur ^ 1], fri_pol[cur], pol_bits, fri_steps[si], sx, shift_inv)) return -1;
                cur ^= 1;
            }
            if (si < fri_steps.size() - 1) {
                uint32_t nb = fri_steps[si + 1];
                uint64_t ngroups = 1ULL << nb;
                uint64_t width = (3ULL << fri_steps[si]) / ngroups;
                // (layer 0 of a prover that keeps f in row blocks: no whole
                // fri_pol[0] exists, the override reads the blocks)
                const uint64_t *pol = si == 0 && !fri_pol0_filled() ? nullptr : fri_pol[cur];
                if (fri_transpose_layer(si, fri_aux[si + 1], pol, 1ULL << fri_steps[si], nb)) return -1;
                if (fri_commit(si + 1, ngroups, width, &fri_roots[4 * (si + 1)])) return -1;
                tr.put(&fri_roots[4 * (si + 1)], 4);
            } else {
                CK(zkgpu_memcpy_d2h(final_pol.data(), fri_pol[cur], final_pol.size() * 8));
                tr.put(final_pol.data(), final_pol.size());
            }
            pol_bits = fri_steps[si];
            for (uint32_t j = 0; j < red; j++) shift_inv = mul(shift_inv, shift_inv);
        }
        if (tstop("STARK_STEP_FRI_FOLDS")) return -1;
        tstart();
        std::vector<uint64_t> ys(q());
        tr.get_permutations(ys.data(), q(), fri_steps[0]);
        pend.clear();
        pend_idx.clear();
        // FRI layers si >= 1: root, vals, siblings
        std::vector<uint64_t> yq = ys;
        for (size_t si = 0; si < fri_steps.size(); si++) {
            if (si > 0) {  // root, then the openings written in place (at flush_opens at the latest)
                uint64_t ngroups = 1ULL << fri_steps[si];
                uint64_t width = (3ULL << fri_steps[si - 1]) / ngroups;
                memcpy(w, &fri_roots[4 * si], 32);
                w += 4;
                uint64_t *vals = w, *sibs = w + q() * width;
                w = sibs + (uint64_t)q() * fri_steps[si] * 4;
                if (fri_open(si, ngroups, width, yq, vals, sibs)) return -1;
            }
            if (si < fri_steps.size() - 1)
                for (auto &y : yq) y %= (1ULL << fri_steps[si + 1]);
        }
        if (open_s0(ys, w) || flush_opens()) return -1;
        memcpy(w, final_pol.data(), final_pol.size() * 8);
        w += final_pol.size();
        if (tstop("STARK_STEP_FRI_QUERIES") || flush_timers()) return -1;
        if (tr.err) return fail("transcript hashing failed: %s", zkgpu_last_error());
        if ((uint64_t)(w - out) != proof_len()) return fail("proof length mismatch");
        timers.emplace_back("STARK_TOTAL", std::chrono::duration<double, std::milli>(clk::now() - tall).count());
        if (exec_commit_ms >= 0) {  // the hand-off that loaded this proof's trace (set_cm1_witness), outside the total
            timers.emplace_back("ZKGPU_EXEC_COMMIT", exec_commit_ms);
            exec_commit_ms = -1.0;
        }
        return 0;
    }

    // fold step si: 2^pol_bits -> 2^out_bits elements (friProve.cpp:44-108)
    virtual int fri_fold_step(size_t si, uint64_t *dst, const uint64_t *src, uint32_t pol_bits, uint32_t out_bits,
                              const uint64_t sx[3], uint64_t shift_inv)
    {
        (void)si;
        CK(zkgpu_fri_fold_dev(dst, src, pol_bits, out_bits, sx, shift_inv));
        return 0;
    }
    // whether fri_pol[0] holds the whole FRI polynomial when the FRI loop
    // starts (the row-sharded prover keeps it in row blocks instead)
    virtual bool fri_pol0_filled() const { return true; }
    // layer si + 1's tree rows: getTransposed of the 2^pol_bits-element
    // polynomial of step si into 2^nb groups (friProve.cpp:111-121)
    virtual int fri_transpose_layer(size_t si, uint64_t *aux, const uint64_t *pol, uint64_t degree, uint32_t nb)
    {
        (void)si;
        CK(zkgpu_fri_transpose_dev(aux, pol, degree, nb));
        return 0;
    }
    // FRI layer si's tree over its ngroups x width row-major groups (friProve.cpp:125-133)
    virtual int fri_commit(size_t si, uint64_t ngroups, uint64_t width, uint64_t root[4])
    {
        CK(zkgpu_gl_merkletree_rows_dev(fri_nodes[si], fri_aux[si], width, ngroups));
        CK(zkgpu_memcpy_d2h(root, fri_nodes[si] + zkgpu_gl_merkle_num_elements(ngroups) - 4, 32));
        return 0;
    }
    // its openings at groups yq (vals q x width, siblings q x log2(ngroups) x 4)
    // (queued: written by flush_opens, all of a proof's openings in one round trip)
    virtual int fri_open(size_t si, uint64_t ngroups, uint64_t width, const std::vector<uint64_t> &yq, uint64_t *vals,
                         uint64_t *sibs)
    {
        pend_idx.emplace_back(yq);
        pend.push_back({vals, sibs, fri_nodes[si], fri_aux[si], 0, width, ngroups, pend_idx.back().data(), q(), 1});
        return 0;
    }

    // s0: the 4 stage trees + the constant tree at the original indices
    // (queued like fri_open): vals of the 5 trees, then their siblings
    virtual int open_s0(const std::vector<uint64_t> &ys, uint64_t *&w)
    {
        const uint32_t secs[5] = {SEC_CM1_2NS, SEC_CM2_2NS, SEC_CM3_2NS, SEC_CM4_2NS, SEC_CONST_2NS};
        const uint32_t widths[5] = {info.n_cm1, info.n_cm2, info.n_cm3, info.n_cm4, info.n_const};
        uint64_t *trees[5] = {nodes[0], nodes[1], nodes[2], nodes[3], const_nodes};
        uint64_t *sib = w;
        for (int t = 0; t < 5; t++) sib += (uint64_t)q() * widths[t];
        pend_idx.emplace_back(ys);
        for (int t = 0; t < 5; t++) {
            pend.push_back({w, sib, trees[t], S.sec[secs[t]], NE, widths[t], NE, pend_idx.back().data(), q(), 0});
            w += (uint64_t)q() * widths[t];
            sib += (uint64_t)q() * info.n_bits_ext * 4;
        }
        w = sib;
        return 0;
    }

    // the queued openings (fri_open / open_s0 of this class)
    std::vector<zkgpu_open_req> pend;
    std::vector<std::vector<uint64_t>> pend_idx;
    int flush_opens()
    {
        const int rc = pend.empty() ? 0 : zkgpu_gl_merkle_open_many(pend.data(), (uint32_t)pend.size());
        pend.clear();
        pend_idx.clear();
        CK(rc);
        return 0;
    }
};

#include "sharded_starks.hpp"

}  // namespace zkgpu_host

#include "comm_host.hpp"
#include "comm_rccl.hpp"

using zkgpu_host::ShardedStarks;
using zkgpu_host::Starks;

extern "C" {

const char *zkgpu_stark_last_error(void) { return zkgpu_host::g_err; }

int zkgpu_stark_create_ex(void **handle, const zkgpu_stark_info *info, uint32_t memory_plan)
{
    Starks *s = new Starks();
    if (s->create(info, memory_plan)) {
        delete s;
        *handle = nullptr;
        return -1;
    }
    *handle = s;
    return 0;
}

int zkgpu_stark_create(void **handle, const zkgpu_stark_info *info)
{
    return zkgpu_stark_create_ex(handle, info, ZKGPU_MEM_AUTO);
}

int zkgpu_stark_memory_mode(void *h) { return ((Starks *)h)->mem_mode; }

int zkgpu_stark_witness(void *h) { return ((Starks *)h)->witness(); }
int zkgpu_stark_set_cm1(void *h, const uint64_t *rows) { return ((Starks *)h)->set_cm1(rows); }
int zkgpu_stark_set_cm1_async(void *h, const uint64_t *rows) { return ((Starks *)h)->set_cm1_async(rows); }
int zkgpu_stark_get_cm1(void *h, uint64_t *rows) { return ((Starks *)h)->get_cm1(rows); }
int zkgpu_stark_set_exec(void *h, const uint64_t *image, uint64_t image_words, uint64_t size_witness)
{
    return ((Starks *)h)->set_exec(image, image_words, size_witness);
}
int zkgpu_stark_set_cm1_witness(void *h, const uint64_t *witness) { return ((Starks *)h)->set_cm1_witness(witness); }
int zkgpu_stark_set_const(void *h, const uint64_t *rows) { return ((Starks *)h)->set_const(rows); }
int zkgpu_stark_set_publics(void *h, const uint64_t *publics) { return ((Starks *)h)->set_publics(publics); }
uint64_t zkgpu_stark_proof_len(void *h) { return ((Starks *)h)->proof_len(); }
int zkgpu_stark_prove(void *h, uint64_t *out) { return ((Starks *)h)->prove(out); }
int zkgpu_stark_prove_from_rows(void *h, const uint64_t *rows, int register_host, uint64_t *out)
{
    return ((Starks *)h)->prove_from_rows(rows, register_host, out);
}
int zkgpu_stark_verkey(void *h, uint64_t out[4])
{
    memcpy(out, ((Starks *)h)->verkey, 32);
    return 0;
}
int zkgpu_stark_publics(void *h, uint64_t *out)
{
    Starks *s = (Starks *)h;
    memcpy(out, s->publics.data(), s->publics.size() * 8);
    return (int)s->publics.size();
}
int zkgpu_stark_timers(void *h, char *names_buf, uint64_t names_len, double *ms, uint32_t max)
{
    Starks *s = (Starks *)h;
    std::string names;
    uint32_t n = 0;
    for (auto &t : s->timers) {
        if (n >= max) break;
        names += t.first + "\n";
        ms[n++] = t.second;
    }
    if (names_len) {
        size_t c = names.size() < names_len - 1 ? names.size() : names_len - 1;
        memcpy(names_buf, names.data(), c);
        names_buf[c] = 0;
    }
    return (int)n;
}
void zkgpu_stark_destroy(void *h) { delete (Starks *)h; }

int zkgpu_stark_probe_set(void *h, const uint64_t *rows_n, uint32_t n_rows_n, const uint64_t *rows_ext,
                          uint32_t n_rows_ext)
{
    return ((Starks *)h)->probe_set(rows_n, n_rows_n, rows_ext, n_rows_ext);
}
int zkgpu_stark_check_set(void *h, uint32_t mode) { return ((Starks *)h)->check_set(mode); }
int zkgpu_stark_check_result(void *h, zkgpu_check_result *out) { return ((Starks *)h)->check_result(out); }
int zkgpu_stark_z_diag(void *h, zkgpu_z_diag *out) { return ((Starks *)h)->z_diag(out); }
int zkgpu_stark_audit(void *h, uint32_t flags, zkgpu_audit_report *out) { return ((Starks *)h)->audit(flags, out); }
int zkgpu_stark_audit_format(void *h, char *buf, uint64_t len) { return ((Starks *)h)->audit_format(buf, len); }
int zkgpu_stark_conn_set(void *h, uint32_t z, const zkgpu_conn_desc *d) { return ((Starks *)h)->conn_set(z, d); }
int zkgpu_stark_conn_check(void *h, uint32_t z, zkgpu_conn_report *out) { return ((Starks *)h)->conn_check(z, out); }
int zkgpu_stark_audit_conn(void *h, uint32_t k, zkgpu_conn_report *out) { return ((Starks *)h)->audit_conn(k, out); }
int zkgpu_stark_check_names_set(void *h, int on) { return ((Starks *)h)->check_names_set(on); }
int zkgpu_stark_check_terms(void *h, zxp_split_term *out, uint32_t max, uint32_t *n)
{
    return ((Starks *)h)->check_terms(out, max, n);
}
int zkgpu_stark_check_named(void *h, uint32_t slot, uint32_t *ids, uint64_t *values, uint32_t max, uint32_t *n_failing)
{
    return ((Starks *)h)->check_named(slot, ids, values, max, n_failing);
}
int zkgpu_stark_probe_size(void *h, uint32_t *n_recs, uint64_t *n_words)
{
    return ((Starks *)h)->probe_size(n_recs, n_words);
}
int zkgpu_stark_probe_read(void *h, zkgpu_probe_rec *recs, uint32_t max_recs, uint64_t *payload, uint64_t max_words)
{
    return ((Starks *)h)->probe_read(recs, max_recs, payload, max_words);
}

// the prover's own Transcript class behind the reference's Transcript surface
struct zkgpu_transcript {
    zkgpu_host::Transcript t;
};
zkgpu_transcript *zkgpu_transcript_create(void) { return new zkgpu_transcript(); }
void zkgpu_transcript_destroy(zkgpu_transcript *t) { delete t; }
int zkgpu_transcript_put(zkgpu_transcript *t, const uint64_t *in, uint64_t n)
{
    if (!t || (n && !in)) return zkgpu_host::fail("transcript_put: null argument");
    t->t.put(in, n);
    return t->t.err ? zkgpu_host::fail("transcript_put: host permutation failed") : 0;
}
int zkgpu_transcript_get_fields1(zkgpu_transcript *t, uint64_t *out)
{
    if (!t || !out) return zkgpu_host::fail("transcript_get_fields1: null argument");
    *out = t->t.get_fields1();
    return t->t.err ? zkgpu_host::fail("transcript_get_fields1: host permutation failed") : 0;
}
int zkgpu_transcript_get_field(zkgpu_transcript *t, uint64_t out[3])
{
    if (!t || !out) return zkgpu_host::fail("transcript_get_field: null argument");
    t->t.get_field(out);
    return t->t.err ? zkgpu_host::fail("transcript_get_field: host permutation failed") : 0;
}
int zkgpu_transcript_get_permutations(zkgpu_transcript *t, uint64_t *res, uint64_t n, uint64_t nbits)
{
    if (!t || (n && !res)) return zkgpu_host::fail("transcript_get_permutations: null argument");
    if (nbits == 0 || nbits > 63) return zkgpu_host::fail("transcript_get_permutations: nbits %lu not in [1, 63]", (unsigned long)nbits);
    if (n == 0) return 0;
    t->t.get_permutations(res, n, nbits);
    return t->t.err ? zkgpu_host::fail("transcript_get_permutations: host permutation failed") : 0;
}

int zkgpu_stark_create_sharded(void **handle, const zkgpu_stark_info *info, const zkgpu_comm *comm)
{
    *handle = nullptr;
    if (!comm) return zkgpu_host::fail("stark_create_sharded: no communicator");
    ShardedStarks *s = new ShardedStarks();
    if (s->create_sharded(info, comm)) {
        delete s;
        return -1;
    }
    *handle = s;
    return 0;
}

int zkgpu_stark_memory_plan(const zkgpu_stark_info *info, uint32_t world, uint64_t *bytes_per_gpu)
{
    if (!info || !bytes_per_gpu) return zkgpu_host::fail("stark_memory_plan: null argument");
    *bytes_per_gpu = 0;
    if (world == 0) {
        Starks s;
        if (s.load(info, false)) return -1;
        return s.plan(bytes_per_gpu);
    }
    ShardedStarks s;
    if (s.shape(info, world, 0, false)) return -1;
    return s.plan(bytes_per_gpu);
}

int zkgpu_stark_memory_plan_ex(const zkgpu_stark_info *info, uint32_t memory_plan, uint64_t *bytes)
{
    if (!info || !bytes) return zkgpu_host::fail("stark_memory_plan_ex: null argument");
    *bytes = 0;
    if (memory_plan > ZKGPU_MEM_LEAN) return zkgpu_host::fail("stark_memory_plan_ex: unknown plan %u", memory_plan);
    Starks s;
    if (s.load(info, false)) return -1;
    if (memory_plan == ZKGPU_MEM_LEAN) {
        std::string why;
        if (!s.lean_ok(why)) return zkgpu_host::fail("stark_memory_plan_ex: the lean plan does not apply: %s", why.c_str());
        s.set_mode(ZKGPU_MEM_LEAN, false);  // (no device: no kept columns)
    }
    return s.plan(bytes);
}

int zkgpu_comm_rccl_unique_id(uint8_t id[128])
{
    using zkgpu_host::g_rccl;
    if (g_rccl.load()) return -1;
    ncclUniqueId u;
    ncclResult_t r = g_rccl.get_unique_id(&u);
    if (r != ncclSuccess) return zkgpu_host::fail("ncclGetUniqueId: %s", g_rccl.error_string(r));
    static_assert(sizeof u == 128, "ncclUniqueId size");
    memcpy(id, &u, 128);
    return 0;
}

int zkgpu_comm_rccl_create(zkgpu_comm *comm, const uint8_t id[128], uint32_t world, uint32_t rank)
{
    using zkgpu_host::g_rccl;
    memset(comm, 0, sizeof *comm);
    if (g_rccl.load()) return -1;
    if (zkgpu_init(-1)) return zkgpu_host::fail("zkgpu_comm_rccl_create: %s", zkgpu_last_error());
    ncclUniqueId u;
    memcpy(&u, id, 128);
    auto *ctx = new zkgpu_host::RcclCtx();
    ncclResult_t r = g_rccl.comm_init_rank(&ctx->comm, (int)world, u, (int)rank);
    if (r != ncclSuccess) {
        delete ctx;
        return zkgpu_host::fail("ncclCommInitRank(world %u, rank %u): %s", world, rank, g_rccl.error_string(r));
    }
    comm->rank = rank;
    comm->world = world;
    comm->ctx = ctx;
    comm->exchange = zkgpu_host::rccl_exchange;
    comm->abort = zkgpu_host::rccl_abort;
    return 0;
}

int zkgpu_comm_host_create(zkgpu_comm *comm, const char *name, uint32_t world, uint32_t rank, uint64_t capacity)
{
    return zkgpu_host::host_comm_create(comm, name, world, rank, capacity);
}

void zkgpu_comm_host_destroy(zkgpu_comm *comm) { zkgpu_host::host_comm_destroy(comm); }

void zkgpu_comm_rccl_destroy(zkgpu_comm *comm)
{
    if (!comm || !comm->ctx) return;
    auto *ctx = (zkgpu_host::RcclCtx *)comm->ctx;
    if (ctx->comm && !ctx->aborted && zkgpu_host::g_rccl.comm_destroy) zkgpu_host::g_rccl.comm_destroy(ctx->comm);
    if (ctx->done) (void)hipEventDestroy(ctx->done);
    delete ctx;
    comm->ctx = nullptr;
    comm->exchange = nullptr;
    comm->abort = nullptr;
}

}  // extern "C"
