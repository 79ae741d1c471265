// Source generator of the run-time compiled expression kernels (hiprtc, the
// code-object cache and the launch: csrc/zxp_jit.hip).  Plain host C++.
//
// A compiled program (csrc/zxp_compile.cpp: fused DOT instructions, SSA temps)
// is printed as one straight-line HIP kernel -- temporaries in registers,
// every column read a coalesced load the compiler can schedule freely, stores
// of columns the program also reads deferred to the end of the row.  Only the
// program STRUCTURE is in the source (column slots, row shifts, table
// offsets); challenge-dependent values (DOT coefficient limbs, F_p^3
// constants) and pointers are kernel inputs.  csrc/gl_device.hpp is embedded
// verbatim, so the field arithmetic is the code the interpreter runs.
//
// Phases, one function each: column slots and written cells (Slots), fused chains
// (detect_chains, unroll_chains), the DOT plan (plan_dots), emission in code blocks and
// limb chunks (emit_body), the chunk-start patch (patch_chunks), assembly with the two
// text passes over the printed body (assemble: lds_column_cache, prefetch_blocks).  The
// limb table kl is appended to by plan_dots, then by emission; kmap re-orders it by
// emission for a split program.
//
// NAMES.  Per-row names, and only they, end in the row suffix _0 (a12_0, D7_1_0, i_0).
// body_bytes() cuts the code blocks by the byte count the block sizes were measured in, in
// which a suffix is one byte, and finds the suffixes in the printed body: a new name or
// literal that ends in _0 without being per-row, or a per-row name without it, silently
// moves every block boundary of the split programs (other kernels, other cache keys).
#include "zxp_jit_source.hpp"

#include <algorithm>
#include <array>
#include <charconv>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <unordered_map>

#include "zxp_segment.hpp"

namespace zk {

static const char *k_gl_device_src =
#include "gl_device_src.inc"
    ;

// DOT limb tables up to this size are staged in LDS per workgroup: read from
// there, the straight-line terms' constants do not compete for the 106 SGPRs
// (scalar loads of every term's limbs hoisted by the scheduler spill SGPRs
// into VGPR lanes -- thousands of v_readlane/v_writelane per row).
constexpr size_t JIT_KL_LDS_MAX = 48 * 1024;
// Limb tables of at least JIT_KL_LDS_MIN words are staged in LDS.  Measured
// on the config-4 STARK at 2^23:
// step42ns (4.1 K words) 14.1 -> 12.4 ms; step52ns (0.4 K words) is
// 9.2 -> 14.4 ms with LDS (its VGPRs go 74 -> 198), so small tables stay on
// scalar loads.
constexpr size_t JIT_KL_LDS_MIN = 1024;
bool jit_kl_lds(size_t nkl) { return nkl >= JIT_KL_LDS_MIN && nkl * 4 <= JIT_KL_LDS_MAX; }

// Segment kernels (round 6, VERDICT r5 "next" 4):
// 512-byte code blocks, up to 16 LDS cache slots per lane (LDS budget
// 160 KB / waves per workgroup, 4 waves per SIMD) and the software prefetch
// below (16 loads, one block ahead).  zkEVM-shaped quotient at 2^24 rows:
// 49.9 -> 56.1 Mrow/s (r06_seg_ab.json).  A/B switch:
// ZKGPU_ZXP_SEG_AB="waves,slots,prefetch[,block bytes[,blocks ahead]]"
// (4,12,0,1024,1 = the round-5 segments).
const SegAb &seg_ab()
{
    static const SegAb c = [] {
        SegAb v;
        if (const char *e = getenv("ZKGPU_ZXP_SEG_AB")) {
            if (sscanf(e, "%u,%u,%u,%u,%u", &v.waves, &v.slots, &v.prefetch, &v.block, &v.dist) < 3 || v.waves > 8)
                v = SegAb();
        }
        return v;
    }();
    return c;
}

namespace {

constexpr uint64_t GL_P = 0xFFFFFFFF00000001ULL;
inline uint64_t gl_add(uint64_t a, uint64_t b)  // canonical a, b
{
    const uint64_t s = a + b;
    return (s < a || s >= GL_P) ? s - GL_P : s;
}
// f(operand) for every operand instruction k reads (a DOT: its terms' sources)
template <class F>
void for_each_read(const ZxpJitIn &in, uint32_t k, F f)
{
    const zxp_instr &I = in.ins[k];
    if (I.op == ZXP_DOT1 || I.op == ZXP_DOT3) {
        for (uint32_t t = I.a; t < I.a + I.b; t++)
            if (in.terms[t].src != ZXP_TERM_ONE) f(in.terms[t].src);
    } else {
        f(I.a);
        if (I.op != ZXP_COPY) f(I.b);
    }
}
constexpr int JIT_KCHUNK = 1024;  // words per LDS limb chunk (256 threads x 16 bytes)

// One row per thread: per-row names carry the suffix _0, ZKJIT_ROWS is 1 (2 rows measured
// equal).  JitTerm / JitParams: as in zxp_jit_source.hpp / zxp_jit.hip.
const char *k_kernel_head = R"(
using namespace zk;
struct JitTerm {
    const uint64_t *ptr;
    int64_t sh;
    uint32_t c[3][6];
    uint32_t pad[2];
};
struct JitParams {
    const uint64_t *const *cp;
    const uint64_t *kc;
    const uint32_t *kl;
    const JitTerm *zt;
    const uint64_t *xdiv, *xdivw, *zh, *tw_lo, *tw_hi;
    uint64_t x_start, rmask;
    uint32_t logdom, logomega, zmask;
    uint32_t nkl;
    uint32_t one;
};
// long column runs of a DOT: a loop over table terms, ZKJIT_UNROLL loads in flight
template <int D>
__device__ __forceinline__ void dot_cols(Dot3 &d0, Dot3 &d1, Dot3 &d2, const JitTerm *t, int n, uint64_t i,
                                         uint64_t m)
{
    constexpr int U = ZKJIT_UNROLL;
    int k = 0;
    for (; k + U <= n; k += U) {
        uint64_t a[U];
#pragma unroll
        for (int u = 0; u < U; u++) a[u] = gload(t[k + u].ptr + ((i + (uint64_t)t[k + u].sh) & m));
#pragma unroll
        for (int u = 0; u < U; u++) {
            d0.term(a[u], t[k + u].c[0]);
            if (D == 3) {
                d1.term(a[u], t[k + u].c[1]);
                d2.term(a[u], t[k + u].c[2]);
            }
        }
    }
    for (; k < n; k++) {
        const uint64_t a = gload(t[k].ptr + ((i + (uint64_t)t[k].sh) & m));
        d0.term(a, t[k].c[0]);
        if (D == 3) {
            d1.term(a, t[k].c[1]);
            d2.term(a, t[k].c[2]);
        }
    }
}
// one 16-byte slice of a limb chunk per thread (256 threads: 1024 words)
__device__ __forceinline__ uint4 kpre(const uint32_t *kl, size_t lo)
{
    return *(const __attribute__((address_space(1))) uint4 *)(kl + lo + 4 * threadIdx.x);
}
__device__ __forceinline__ void kput(uint32_t *dst, uint4 v) { *(uint4 *)(dst + 4 * threadIdx.x) = v; }
__device__ __forceinline__ uint64_t gload_o(const uint64_t *base, uint32_t byte_off)
{
    return *(const gu64_t *)((const char *)base + byte_off);
}
__device__ __forceinline__ uint64_t zk_cs(uint64_t *slot, uint64_t v)
{
    *slot = v;
    return v;
}
__device__ __forceinline__ int zk_one()
{
    int c;
    asm volatile("s_mov_b32 %0, 1" : "=s"(c));
    return c;
}
extern "C" __global__ void __launch_bounds__(256) ZKJIT_WAVES zxp_jit(const JitParams p)
{
#if ZKJIT_KL_LDS
    extern __shared__ __attribute__((aligned(16))) uint32_t kls[];
    for (uint32_t w = threadIdx.x; w < p.nkl; w += 256) kls[w] = p.kl[w];
    const uint32_t *K = kls;
#else
    const uint32_t *K = p.kl;
#endif
    const JitTerm *ZT = p.zt;  // (in LDS: measured slower, 9.0 -> 11.4 ms for step52ns)
#if ZKJIT_KL_LDS
    __syncthreads();
#endif
    // ZKJIT_ROWS rows per thread: i_r = ib_ + r * S_ (each row set is
    // contiguous over the lanes, so every column load stays coalesced)
    const uint64_t S_ = (1ULL << p.logdom) / ZKJIT_ROWS;
#if ZKJIT_KL_CHUNK
    // limb chunks staged in LDS per code block (workgroup barriers: every
    // thread stays to the end, rows past the domain only skip the stores)
    const uint64_t i_ = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live_ = i_ < S_;
    const uint64_t ib_ = live_ ? i_ : 0;
    __shared__ __attribute__((aligned(16))) uint32_t kbuf[2 * ZKJIT_KL_CHUNK];
    uint4 pf_;  // the next chunk, in flight (zxp_jit_source chunk_head)
    kput(kbuf, kpre(p.kl, 0));
    __syncthreads();
#else
    const uint64_t ib_ = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (ib_ >= S_) return;
#endif
    const uint64_t m = p.rmask;
#ifdef ZK_CP_AS
#define CPTR(j) ((uint64_t *)(((const ZK_CP_AS uint64_t *)p.cp)[j]))
#else
#define CPTR(j) (const_cast<uint64_t *>(p.cp[j]))
#endif
// a column read: 32-bit byte offset from the column's (scalar) base, so the
// load takes the global_load saddr form -- one offset register per row shift
// shared by every column, no 64-bit address per load (domains <= 2^28 rows,
// api.hip use_jit)
#if ZKJIT_SADDR
const uint32_t m32_ = (uint32_t)m;
#define C(j, sh, ii) gload_o(CPTR(j), (((uint32_t)(ii) + (uint32_t)(sh)) & m32_) << 3)
#else
#define C(j, sh, ii) gload(CPTR(j) + ((ii + (uint64_t)(sh)) & m))
#endif
#if ZKJIT_LCACHE
    // compiler-managed column cache (lds_column_cache): slot s of this lane
    // (ZKJIT_ROWS rows per thread: slot s of row r at (s ROWS + r))
    __shared__ uint64_t zkc[ZKJIT_LCACHE * ZKJIT_ROWS * 256];
    uint64_t *const zkc_ = zkc + threadIdx.x;
#define LC(s, r) (zkc_[((s) * ZKJIT_ROWS + (r)) * 256])
#define CS(j, sh, ii, s, r) zk_cs(zkc_ + ((s) * ZKJIT_ROWS + (r)) * 256, C(j, sh, ii))
#endif
// scratch columns of a segmented program (csrc/zxp_segment.hpp) are stored
// where the value is defined, not deferred to the end of the row
#if ZKJIT_KL_CHUNK
#define ZK_ST(j, v, ii) do { if (live_) gstore_out(CPTR(j) + ii, gl_canon(v)); } while (0)
#define ZK_STS(j, v, ii, sh) do { if (live_) gstore_out(CPTR(j) + ((ii + (uint64_t)(int64_t)(sh)) & m), gl_canon(v)); } while (0)
#else
#define ZK_ST(j, v, ii) gstore_out(CPTR(j) + ii, gl_canon(v))
#define ZK_STS(j, v, ii, sh) gstore_out(CPTR(j) + ((ii + (uint64_t)(int64_t)(sh)) & m), gl_canon(v))
#endif
// a global limb table is re-based in every code block (an opaque copy of K):
// with thousands of loads off one base register, SIFoldOperands dominated
// the compile (48 s of 100 for step3prev)
#if ZKJIT_KL_LDS
#define ZK_KREFRESH
#else
#define ZK_KREFRESH asm volatile("" : "+s"(K));
#endif
)";

void appendf(std::string &s, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    int n = vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (n >= (int)sizeof(buf)) {
        std::vector<char> big(n + 1);
        va_start(ap, fmt);
        vsnprintf(big.data(), big.size(), fmt, ap);
        va_end(ap);
        s += big.data();
    } else {
        s += buf;
    }
}

inline bool ident(char c) { return (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z') || (c >= '0' && c <= '9') || c == '_'; }
// decimal text without the printf machinery (the per-term lines below are
// ~10 K appends per segment: vsnprintf was ~60 % of a segment's source time)
inline void app_num(std::string &s, uint64_t v)
{
    char b[24];
    const auto r = std::to_chars(b, b + sizeof(b), v);
    s.append(b, r.ptr);
}

// one DOT term's line: D<dot>_j_0.term_al(<val>, K + <kt + 8 j>) for the
// components of the accumulator (names: see NAMES at the top)
inline void app_term(std::string &s, const std::string &val, uint32_t dot, size_t kt, bool three)
{
    if (three) {
        s += "{ const uint64_t v_ = ";
        s += val;
        for (int j = 0; j < 3; j++) {
            s += j ? " D" : "; D";
            app_num(s, dot);
            s += j == 0 ? "_0_0.term_al(v_, K + " : j == 1 ? "_1_0.term_al(v_, K + " : "_2_0.term_al(v_, K + ";
            app_num(s, kt + 8 * (size_t)j);
            s += ");";
        }
        s += " }\n";
    } else {
        s += 'D';
        app_num(s, dot);
        s += "_0_0.term_al(";
        s += val;
        s += ", K + ";
        app_num(s, kt);
        s += ");\n";
    }
}

// ---- the text passes.  Every column read of a printed body is a token
// C(j,sh,i_0) (CS(j,sh,i_0,s,0) once cached), in emission order, one statement
// per line; an immediate store names its column first, ZK_ST(j / ZK_STS(j.
struct ColRead {
    size_t pos, len;  // the token's text
    uint32_t col;     // cp slot j
    int32_t sh, slot;  // slot: the cache slot of a CS, else -1
    uint32_t line;
    uint64_t key() const { return ((uint64_t)col << 32) | (uint32_t)sh; }
};
struct BodyScan {
    std::vector<ColRead> reads;
    std::set<uint32_t> stored;
};
static BodyScan scan_body(const std::string &body)
{
    auto num = [](const char *&t, int64_t &v) {
        char *e;
        v = strtoll(t, &e, 10);
        const bool ok = e != t;
        t = e;
        return ok;
    };
    BodyScan s;
    uint32_t line = 0;
    const char *bp = body.c_str();
    for (size_t q = 0, bn = body.size(); q < bn; q++) {
        const char ch = bp[q];
        if (ch == '\n') line++;
        if ((ch != 'C' && ch != 'Z') || (q > 0 && ident(bp[q - 1]))) continue;
        const char *t = bp + q;
        int64_t j, sh, slot = -1;
        if (ch == 'Z') {
            if (!strncmp(t, "ZK_ST(", 6) || !strncmp(t, "ZK_STS(", 7)) {
                t += t[5] == 'S' ? 7 : 6;
                if (num(t, j)) s.stored.insert((uint32_t)j);
            }
            continue;
        }
        const bool cs = t[1] == 'S';
        if (t[cs ? 2 : 1] != '(') continue;
        t += cs ? 3 : 2;
        if (!num(t, j) || *t++ != ',' || !num(t, sh) || strncmp(t, ",i_0", 4)) continue;
        t += 4;
        if (cs) {
            if (*t++ != ',' || !num(t, slot) || strncmp(t, ",0", 2)) continue;
            t += 2;
        }
        if (*t++ != ')') continue;
        s.reads.push_back({q, (size_t)(t - bp) - q, (uint32_t)j, (int32_t)sh, (int32_t)slot, line});
    }
    return s;
}

// Software prefetch across code blocks (the SEG_AB experiment): the first
// `pf` global column reads of every code block are issued at the start of the
// block before it, into per-row registers (zpf<k>_0), and read from there --
// a column load then has a whole code block (~1 KB of source) to arrive
// instead of the compiler's in-block scheduling window.  Loads stay
// in flight across __syncthreads (it waits for LDS only).  Columns the kernel
// stores to are never prefetched; a cached read (CS) keeps its slot store.
// Returns the number of prefetch registers.
static uint32_t prefetch_blocks(std::string &body, uint32_t pf, uint32_t dist = 1)
{
    static const std::string head = "if (zk_one()) {\n";
    std::vector<size_t> starts;
    for (size_t q = body.find(head); q != std::string::npos; q = body.find(head, q + head.size()))
        starts.push_back(q + head.size());
    if (starts.size() < 2 || !pf) return 0;
    const BodyScan scan = scan_body(body);
    struct Edit {
        size_t pos, len;
        std::string text;
    };
    std::vector<Edit> edits;  // replacements and insertions, by position
    uint32_t n = 0;
    size_t r = 0;  // reads, in order of position
    for (size_t b = 1; b < starts.size(); b++) {
        const size_t lo = starts[b], hi = b + 1 < starts.size() ? starts[b + 1] - head.size() : body.size();
        std::string loads;
        uint32_t taken = 0;
        while (r < scan.reads.size() && scan.reads[r].pos < lo) r++;
        for (; r < scan.reads.size() && scan.reads[r].pos < hi && taken < pf; r++) {
            const ColRead &x = scan.reads[r];
            if (scan.stored.count(x.col)) continue;
            std::string var = "zpf";
            app_num(var, n);
            var += "_0";
            loads += var + " = C(";
            loads += std::to_string(x.col) + "," + std::to_string(x.sh) + ",i_0);\n";
            edits.push_back({x.pos, x.len, x.slot >= 0 ? "CSV(" + var + "," + std::to_string(x.slot) + ",0)" : var});
            n++;
            taken++;
        }
        if (!loads.empty()) edits.push_back({starts[b >= dist ? b - dist : 0], 0, loads});
    }
    std::stable_sort(edits.begin(), edits.end(), [](const Edit &x, const Edit &y) { return x.pos < y.pos; });
    std::string out;
    out.reserve(body.size() + n * 40);
    size_t at = 0;
    for (const Edit &e : edits) {
        out.append(body, at, e.pos - at);
        out += e.text;
        at = e.pos + e.len;
    }
    out.append(body, at, std::string::npos);
    body.swap(out);
    return n;
}

// Compiler-managed LDS column cache for block-split programs.  A large
// program's kernel is HBM-bound on re-reads: it loads a column again at every
// use, and a re-read hits the 4 MB L2 of an XCD only within ~16 columns (512
// waves x 512 bytes per column in flight).  The whole read
// sequence is known here, so each lane keeps up to `slots` column values in
// LDS chosen by Belady's rule (on a miss, evict the value whose next read is
// furthest away, or bypass when the new value's next read is further still):
// a read of a cached value becomes an LDS read, LC(s,0), and a read that enters
// the cache stores its value as it loads it, CS(..., s,0).  The body is
// rewritten textually (scan_body).  Within a line the operand evaluation order
// is unspecified, so a slot read or filled on a line is not evicted on that
// line.  Columns the kernel stores to are never cached.  Returns the number
// of cached reads (LDS hits).
static size_t lds_column_cache(std::string &body, int slots)
{
    const BodyScan scan = scan_body(body);
    const std::vector<ColRead> &rd = scan.reads;
    const uint64_t INF = ~0ULL;
    std::vector<uint64_t> nx(rd.size(), INF);
    {
        std::unordered_map<uint64_t, size_t> last;
        last.reserve(rd.size());
        for (size_t r = rd.size(); r-- > 0;) {
            auto it = last.find(rd[r].key());
            if (it != last.end()) nx[r] = it->second;
            last[rd[r].key()] = r;
        }
    }
    std::vector<uint64_t> slot_key(slots, INF), slot_nu(slots, INF);
    std::unordered_map<uint64_t, int> where;
    std::vector<int> act(rd.size(), -1), hit(rd.size(), 0);
    std::vector<uint32_t> pinned_line(slots, UINT32_MAX);
    size_t hits = 0;
    for (size_t r = 0; r < rd.size(); r++) {
        const ColRead &x = rd[r];
        if (scan.stored.count(x.col)) continue;
        auto it = where.find(x.key());
        if (it != where.end()) {
            const int sl = it->second;
            act[r] = sl;
            hit[r] = 1;
            hits++;
            pinned_line[sl] = x.line;
            slot_nu[sl] = nx[r];
            if (nx[r] == INF) {  // last read: the slot is free again
                where.erase(it);
                slot_key[sl] = INF;
            }
            continue;
        }
        if (nx[r] == INF) continue;
        int v = -1;
        for (int sl = 0; sl < slots; sl++) {
            if (pinned_line[sl] == x.line) continue;
            if (slot_key[sl] == INF) {
                v = sl;
                break;
            }
            if (v < 0 || slot_nu[sl] > slot_nu[v]) v = sl;
        }
        if (v < 0 || (slot_key[v] != INF && slot_nu[v] <= nx[r])) continue;  // bypass
        if (slot_key[v] != INF) where.erase(slot_key[v]);
        slot_key[v] = x.key();
        slot_nu[v] = nx[r];
        where[x.key()] = v;
        pinned_line[v] = x.line;
        act[r] = v;
    }
    if (!hits) return 0;
    std::string out;
    out.reserve(body.size() + rd.size() * 4);
    size_t at = 0;
    for (size_t r = 0; r < rd.size(); r++) {
        if (act[r] < 0) continue;
        out.append(body, at, rd[r].pos - at);
        out += hit[r] ? "LC(" : "CS(";
        if (!hit[r]) out.append(body, rd[r].pos + 2, rd[r].len - 3) += ',';
        app_num(out, (uint64_t)act[r]);
        out += ",0)";
        at = rd[r].pos + rd[r].len;
    }
    out.append(body, at, std::string::npos);
    body.swap(out);
    return hits;
}

// ---- phase 1: column slots and written cells.  Reads the program; appends to
// cp (a slot is allocated where a phase first asks for it: the order of the calls is part of the output).
struct Slots {
    const ZxpJitIn &in;
    std::vector<const uint64_t *> &cp;
    // (section, col) -> cp slot: a flat table per section (a segment looks up
    // ~10^4 column reads), a map for out-of-table indices
    std::vector<std::vector<uint32_t>> slot_of;
    std::map<std::pair<uint32_t, uint32_t>, uint32_t> slot_far;
    // Columns the program reads (any shift): a written column it never reads
    // is stored where the value is assigned (the compiled program forwards
    // every read of a cell the row wrote, zxp_compile.cpp); a written column
    // it also reads keeps its value in a register w<r> stored at the end of
    // the row, landing on row (i + shift) & m (reads before the write see the
    // old value).  Immediate stores keep the stage-3 programs' ~300 written
    // cells out of the registers.
    std::set<std::pair<uint32_t, uint32_t>> read_cols;
    std::map<std::pair<uint32_t, int32_t>, uint32_t> wreg;
    std::vector<std::pair<uint32_t, int32_t>> wcell;  // register -> (slot, shift)
    std::vector<uint8_t> written_any;                  // per slot, at any shift
    std::vector<uint8_t> wlive;                        // written so far (in program order; set by emission)

    Slots(const ZxpJitIn &in_, std::vector<const uint64_t *> &cp_) : in(in_), cp(cp_), slot_of(ZXP_SEC_SCRATCH + 1)
    {
        auto note = [&](uint32_t o) {
            if (o >= in.n_opnd) return;
            const zxp_operand &x = in.opnd[o];
            if (x.kind == ZXP_COL || x.kind == ZXP_COL3)
                for (uint32_t c = 0; c < (x.kind == ZXP_COL3 ? 3u : 1u); c++) read_cols.insert({x.a, x.b + c});
        };
        for (uint32_t k = 0; k < in.n_instr; k++) for_each_read(in, k, note);
        for (uint32_t k = 0; k < in.n_instr; k++) {
            const zxp_operand &d = in.opnd[in.ins[k].dst];
            if ((d.kind == ZXP_COL || d.kind == ZXP_COL3) && d.a != ZXP_SEC_SCRATCH && !store_now(d.a, d.b))
                for (uint32_t c = 0; c < (d.kind == ZXP_COL3 ? 3u : 1u); c++) {
                    const uint32_t j = slot(d.a, d.b + c);
                    const auto key = std::make_pair(j, (int32_t)d.c);
                    if (!wreg.count(key)) {
                        wreg[key] = (uint32_t)wcell.size();
                        wcell.push_back(key);
                    }
                    if (j >= written_any.size()) written_any.resize(j + 1, 0);
                    written_any[j] = 1;
                }
        }
        wlive.assign(wcell.size(), 0);
    }
    const uint64_t *ptr(uint32_t sec, uint32_t col) const
    {
        if (sec == ZXP_SEC_SCRATCH) return in.scratch + (uint64_t)col * in.scratch_ld;
        return in.sections->sec[sec] + (uint64_t)col * in.sections->ld[sec];
    }
    uint32_t slot(uint32_t sec, uint32_t col)
    {
        if (sec <= ZXP_SEC_SCRATCH && col < (1u << 20)) {
            std::vector<uint32_t> &v = slot_of[sec];
            if (col >= v.size()) v.resize(col + 1, UINT32_MAX);
            if (v[col] == UINT32_MAX) {
                cp.push_back(ptr(sec, col));
                v[col] = (uint32_t)cp.size() - 1;
            }
            return v[col];
        }
        auto key = std::make_pair(sec, col);
        auto it = slot_far.find(key);
        if (it != slot_far.end()) return it->second;
        cp.push_back(ptr(sec, col));
        return slot_far[key] = (uint32_t)cp.size() - 1;
    }
    bool store_now(uint32_t sec, uint32_t col) const { return sec != ZXP_SEC_SCRATCH && !read_cols.count({sec, col}); }
    bool is_written(uint32_t j) const { return j < written_any.size() && written_any[j]; }
    // the register of cell (slot j, shift sh) once the row has written it, else -1
    int64_t live_reg(uint32_t j, int32_t sh) const
    {
        auto it = wreg.find(std::make_pair(j, sh));
        return it != wreg.end() && wlive[it->second] ? (int64_t)it->second : -1;
    }
};

// ---- phases 2 and 3: fused column chains (the FRI polynomial, step52ns) ---
// A Horner chain over committed columns compiles to a chain of DOTs of at
// most max_terms terms, each carrying the previous one as an F_p^3 term;
// the FRI polynomial has one chain per opening point and most columns sit
// in several of them (zkEVM-shaped step52ns: 3 chains, 3,778 column terms
// over 1,497 columns; config-4: 397 over 189), each read again from HBM
// at a distance no cache holds.  A non-split program evaluates up to
// FUSE_MAX such chains together where the first link stood: each chain is
// unrolled on the host (a link's column coefficient mapped through the
// later links' carry maps, exact arithmetic mod p), the columns are
// grouped by the set of chains they appear in, and each group is one loop
// that reads a column once and accumulates it into all of its chains.
// Same values (the chain sum is linear; accumulators are reduced every
// FUSE_PIECE columns).  Measured (A/B on one box): zkEVM-shaped FRI
// polynomial at 2^23 rows 69.4 -> 38.4 ms with 4 column loads in flight
// per iteration, 33.5 ms with 8 (FUSE_U); the config-4 one
// (397 column terms) 9.3 -> 10.4 ms with 4, 8.1 ms with 8.  Small chains
// inside other programs (config-4 quotient, step3prev: 20-24 columns)
// ran slower fused, so a program is fused only when its chains hold at
// least half of its column terms and FUSE_MIN (128) or more -- the FRI
// polynomials.
constexpr int FUSE_MAX = 4;
constexpr uint32_t FUSE_PIECE = 224;
constexpr size_t FUSE_MIN = 128;
constexpr size_t FUSE_U = 8;  // column loads in flight per fused-loop iteration
struct FusedCol {
    uint32_t slot;
    int32_t sh;
    uint32_t mask;  // chains the column appears in (structure, not values)
    uint64_t c[FUSE_MAX][3];
};
struct FusedChains {
    std::vector<int32_t> fused;               // per instruction: chain of a fused link, else -1
    std::vector<std::vector<uint32_t>> links;  // links in order, per fused chain
    uint32_t at = UINT32_MAX;                 // where the fused chains are evaluated
    // unrolled (unroll_chains): per chain, the coefficient (F_p^3) of every
    // column and the constant, mapped through the later links' carry maps
    std::vector<FusedCol> cols;  // in order of first appearance
    std::vector<std::array<uint64_t, 3>> konst;
};

static bool col_term(const ZxpJitIn &in, const zxp_term &tm)
{
    return tm.src != ZXP_TERM_ONE && in.opnd[tm.src].kind == ZXP_COL;
}

// Phase 2.  Reads the program and the written slots; prints nothing.
static FusedChains detect_chains(const ZxpJitIn &in, Slots &sl)
{
    FusedChains fc;
    fc.fused.assign(in.n_instr, -1);
    // a link: DOT3 whose terms are column reads (columns the program never
    // writes), constants, and the whole previous link (its only reader)
    std::map<uint32_t, uint32_t> def_at;  // SSA operand -> defining instruction
    for (uint32_t k = 0; k < in.n_instr; k++) def_at[in.ins[k].dst] = k;
    std::vector<int64_t> prev(in.n_instr, -2);  // -2 not a link, -1 first link, else previous link
    std::vector<uint32_t> readers(in.n_opnd ? in.n_opnd : 1, 0);
    for (uint32_t k = 0; k < in.n_instr; k++) {  // (an instruction counts once per operand it reads)
        std::set<uint32_t> srcs;
        for_each_read(in, k, [&](uint32_t s) { srcs.insert(s); });
        for (uint32_t x : srcs)
            if (x < in.n_opnd) readers[x]++;
    }
    for (uint32_t k = 0; k < in.n_instr; k++) {
        const zxp_instr &I = in.ins[k];
        if (I.op != ZXP_DOT3 || in.opnd[I.dst].kind != ZXP_TMP3) continue;
        int64_t pv = -1;
        bool ok = true;
        uint32_t ncol = 0;
        for (uint32_t t = I.a; t < I.a + I.b && ok; t++) {
            const zxp_term &tm = in.terms[t];
            if (tm.src == ZXP_TERM_ONE) continue;
            const zxp_operand &o = in.opnd[tm.src];
            if (o.kind == ZXP_COL) {
                ok = !sl.is_written(sl.slot(o.a, o.b));
                ncol++;
            } else if (o.kind == ZXP_TMP3 && def_at.count(tm.src) && prev[def_at[tm.src]] != -2 &&
                       readers[tm.src] == 1 && (pv < 0 || pv == (int64_t)def_at[tm.src])) {
                pv = def_at[tm.src];
            } else {
                ok = false;
            }
        }
        if (ok && (ncol > 0 || pv >= 0)) prev[k] = pv;
    }
    // chains: from links nobody continues, walk back
    std::vector<uint8_t> continued(in.n_instr, 0);
    for (uint32_t k = 0; k < in.n_instr; k++)
        if (prev[k] >= 0) continued[prev[k]] = 1;
    std::vector<std::vector<uint32_t>> cand;
    for (uint32_t k = 0; k < in.n_instr; k++) {
        if (prev[k] == -2 || continued[k]) continue;
        std::vector<uint32_t> ch;
        for (int64_t x = k; x >= 0; x = prev[x]) ch.push_back((uint32_t)x);
        std::reverse(ch.begin(), ch.end());
        cand.push_back(ch);
    }
    // the largest chains (by column terms), if at least two share columns
    auto ncols_of = [&](const std::vector<uint32_t> &ch) {
        size_t n = 0;
        for (uint32_t x : ch) n += in.ins[x].b;
        return n;
    };
    std::stable_sort(cand.begin(), cand.end(),
                     [&](const std::vector<uint32_t> &a, const std::vector<uint32_t> &b) { return ncols_of(a) > ncols_of(b); });
    if (cand.size() > (size_t)FUSE_MAX) cand.resize(FUSE_MAX);
    std::map<std::pair<uint32_t, int32_t>, uint32_t> in_chains;  // (slot, shift) -> chain mask
    for (size_t g = 0; g < cand.size(); g++)
        for (uint32_t x : cand[g])
            for (uint32_t t = in.ins[x].a; t < in.ins[x].a + in.ins[x].b; t++) {
                if (!col_term(in, in.terms[t])) continue;
                const zxp_operand &o = in.opnd[in.terms[t].src];
                in_chains[{sl.slot(o.a, o.b), (int32_t)o.c}] |= 1u << g;
            }
    size_t shared = 0, terms = 0, all_terms = 0;
    for (auto &kv : in_chains) {
        shared += __builtin_popcount(kv.second) > 1;
        terms += __builtin_popcount(kv.second);
    }
    for (uint32_t k = 0; k < in.n_instr; k++)  // the program's column terms
        if (in.ins[k].op == ZXP_DOT1 || in.ins[k].op == ZXP_DOT3)
            for (uint32_t t = in.ins[k].a; t < in.ins[k].a + in.ins[k].b; t++) all_terms += col_term(in, in.terms[t]);
    if (cand.size() >= 2 && shared > 0 && terms >= FUSE_MIN && 2 * terms >= all_terms) {
        fc.links = cand;
        for (size_t g = 0; g < fc.links.size(); g++)
            for (uint32_t x : fc.links[g]) {
                fc.fused[x] = (int32_t)g;
                fc.at = std::min(fc.at, x);
            }
    }
    return fc;
}

// Phase 3.  Reads the chains' terms; fills fc.cols and fc.konst (mod p).
static void unroll_chains(const ZxpJitIn &in, Slots &sl, FusedChains &fc)
{
    fc.konst.assign(fc.links.size(), std::array<uint64_t, 3>{0, 0, 0});
    std::map<std::pair<uint32_t, int32_t>, size_t> fidx;
    for (size_t g = 0; g < fc.links.size(); g++)
        for (uint32_t x : fc.links[g])
            for (uint32_t t = in.ins[x].a; t < in.ins[x].a + in.ins[x].b; t++) {
                if (!col_term(in, in.terms[t])) continue;
                const zxp_operand &o = in.opnd[in.terms[t].src];
                const std::pair<uint32_t, int32_t> key{sl.slot(o.a, o.b), (int32_t)o.c};
                if (!fidx.count(key)) {
                    fidx[key] = fc.cols.size();
                    fc.cols.push_back(FusedCol{key.first, key.second, 0, {}});
                }
            }
    for (size_t g = 0; g < fc.links.size(); g++) {
        // M: the map from a link's value to the chain's final value (3x3 over F_p)
        uint64_t M[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
        for (size_t li = fc.links[g].size(); li-- > 0;) {
            const zxp_instr &I = in.ins[fc.links[g][li]];
            uint64_t L[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};  // previous link -> this link
            for (uint32_t t = I.a; t < I.a + I.b; t++) {
                const zxp_term &tm = in.terms[t];
                uint64_t a[3], v[3] = {0, 0, 0};
                for (int j = 0; j < 3; j++) a[j] = tm.coef[j] % GL_P;
                for (int r = 0; r < 3; r++)
                    for (int j = 0; j < 3; j++) v[r] = gl_add(v[r], h_mul(M[r][j], a[j]));
                if (tm.src == ZXP_TERM_ONE) {
                    for (int r = 0; r < 3; r++) fc.konst[g][r] = gl_add(fc.konst[g][r], v[r]);
                } else if (in.opnd[tm.src].kind == ZXP_COL) {
                    const zxp_operand &o = in.opnd[tm.src];
                    FusedCol &c = fc.cols[fidx[{sl.slot(o.a, o.b), (int32_t)o.c}]];
                    c.mask |= 1u << g;
                    for (int r = 0; r < 3; r++) c.c[g][r] = gl_add(c.c[g][r], v[r]);
                } else {  // the previous link, component tm.comp
                    for (int r = 0; r < 3; r++) L[r][tm.comp] = gl_add(L[r][tm.comp], a[r]);
                }
            }
            uint64_t M2[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
            for (int r = 0; r < 3; r++)
                for (int c = 0; c < 3; c++)
                    for (int j = 0; j < 3; j++) M2[r][c] = gl_add(M2[r][c], h_mul(M[r][j], L[j][c]));
            memcpy(M, M2, sizeof(M));
        }
    }
}

struct Expr {
    std::string e;
    int dim;
};
struct Stream {  // a term accumulated where its source temporary is defined (plan_dots)
    uint32_t dot;
    bool three;
    std::string val;
    size_t kt;
};

struct Generator {
    const ZxpJitIn &in;
    ZxpJitSource &o;  // the tables cp / kc / kl / zt grow through the phases
    Slots sl;
    // Only programs of 1000 compiled instructions or more are split: the
    // opaque branch costs registers (config-4 FRI polynomial: 74 -> 200
    // VGPRs, 9 -> 57 ms), and small programs compile in seconds as one block.
    // Limb chunks in LDS, every split program: a split program whose limb
    // table is too large for LDS reads it from global memory, one wave-uniform
    // 16 + 8-byte vector load pair per term, each taking the texture
    // addresser's full 64-lane path.  In this mode the table is rewritten in
    // emission order (kmap), every code block's limbs form one contiguous
    // chunk of <= JIT_KCHUNK words, the workgroup copies the next block's
    // chunk into the other half of an LDS double buffer (one 16-byte load per
    // thread, issued at the block's start) and a barrier closes each block.
    // Quarter-size step42ns-shaped program at 2^24 rows: 251 -> 189 ms
    // (global vector loads of the limbs 25 K -> 6.7 K per wave).
    const bool split;
    FusedChains ch;
    // the plan (plan_dots)
    std::vector<std::vector<Stream>> stream;  // per instruction: the terms accumulated after it
    std::vector<uint8_t> streamed_term;       // per DOT term index: accumulated at the source's definition
    std::vector<size_t> dot_k0;               // per DOT: its constants' limbs in kl
    std::vector<std::vector<uint32_t>> declare_at;  // per instruction: the DOTs whose accumulators open there
    // emission
    std::string body, dot_decls;  // (accumulators are declared at function scope: the body is split into blocks)
    bool uses_x = false;
    size_t block;  // source bytes per code block
    std::vector<uint32_t> kl2;  // kl in emission order (split programs)
    size_t blk_lo = 0, blk_no = 0, block_start = 0;
    size_t suffixes = 0, counted = 0;  // body_bytes
    std::vector<size_t> klo_of;  // chunk start of chunk b

    Generator(const ZxpJitIn &i, ZxpJitSource &s) : in(i), o(s), sl(i, s.cp), split(i.n_instr >= 1000 || i.force_split) {}

    // limb table layout: Dot3 inits 3 words in 4-word slots, terms 6 words in
    // 8-word slots, so the kernel reads them with 16-byte vector loads
    void align_kl(size_t a) { o.kl.resize((o.kl.size() + a - 1) / a * a, 0); }
    void limbs3(uint64_t c)  // Dot3 constant init: 22/21/21-bit limbs of c
    {
        o.kl.insert(o.kl.end(), {(uint32_t)(c & ((1u << 22) - 1)), (uint32_t)((c >> 22) & ((1u << 21) - 1)), (uint32_t)(c >> 43), 0u});
    }
    size_t limbs6x3(const uint64_t coef[3])  // term limbs of the three components; returns the slot
    {
        align_kl(8);
        const size_t kt = o.kl.size();
        for (int j = 0; j < 3; j++) {
            uint32_t l8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            zxp_limbs6(coef[j] % GL_P, l8);
            o.kl.insert(o.kl.end(), l8, l8 + 8);
        }
        return kt;
    }
    std::string tmp_name(const zxp_term &tm) const  // a DOT term's temporary source
    {
        return in.opnd[tm.src].kind == ZXP_TMP1 ? "a" + std::to_string(tm.src) + "_0"
                                                : "b" + std::to_string(tm.src) + "_0.v[" + std::to_string(tm.comp) + "]";
    }

    // ---- phase 4: the DOT plan.  Reads the program and the chains; appends to
    // kl every DOT's constants and its streamed terms, in program order.
    // A term whose source is a temporary is accumulated right where
    // that temporary is defined (exact integer sums commute), so temporaries
    // feeding a linear combination die at once instead of staying live until
    // the DOT: register pressure stays that of one constraint at a time.
    // Streaming a term opens the DOT's accumulators (3 or 9 words) at the
    // source's definition: for a source defined long before its DOT that
    // holds more registers than keeping the source (1 or 3 words) -- the
    // fork-9 step42ns peaked at ~1,300 live words with unbounded streaming
    // against ~110 without.  Only sources defined at most stream_span
    // instructions before their DOT are streamed.
    // Small programs (< 1,000 compiled instructions: one or two Horner
    // accumulators over the whole program) stream without limit.
    // Large programs (block-split) choose per DOT where to open its
    // accumulators by a register cost (open_point).
    void plan_dots()
    {
        const int64_t stream_span = in.n_instr < 1000 ? INT64_MAX / 4 : 24;
        const bool cost_stream = split;
        stream.resize(in.n_instr);
        dot_k0.assign(in.n_instr, 0);
        uint32_t nt = 0;
        std::vector<int64_t> last_read(in.n_opnd ? in.n_opnd : 1, -1);  // per SSA operand
        for (uint32_t k = 0; k < in.n_instr; k++) {
            if (in.ins[k].op == ZXP_DOT1 || in.ins[k].op == ZXP_DOT3) nt = std::max(nt, in.ins[k].a + in.ins[k].b);
            for_each_read(in, k, [&](uint32_t s) {
                if (s < last_read.size()) last_read[s] = k;
            });
        }
        streamed_term.assign(nt, 0);
        std::vector<uint32_t> first_use(in.n_instr, UINT32_MAX);  // declaration point of DOT k's accumulators
        std::vector<int64_t> last1(in.n_tmp1 + 1, -1), last3(in.n_tmp3 + 1, -1);
        // definition of a term's temporary source (-1: never written, the value is 0), -2: not a temporary
        auto def_of = [&](const zxp_term &tm) -> int64_t {
            if (tm.src == ZXP_TERM_ONE) return -2;
            const zxp_operand &s = in.opnd[tm.src];
            return s.kind == ZXP_TMP1 ? last1[s.a] : s.kind == ZXP_TMP3 ? last3[s.a] : -2;
        };
        for (uint32_t k = 0; k < in.n_instr; k++) {
            const zxp_instr &I = in.ins[k];
            const zxp_operand &D = in.opnd[I.dst];
            if (ch.fused[k] >= 0) {  // evaluated with its chain at ch.at
                if (D.kind == ZXP_TMP3) last3[D.a] = (k == ch.links[ch.fused[k]].back()) ? (int64_t)ch.at : (int64_t)k;
                continue;
            }
            if (I.op == ZXP_DOT1 || I.op == ZXP_DOT3) {
                const bool three = I.op == ZXP_DOT3;
                uint64_t c0[3] = {0, 0, 0};
                for (uint32_t t = I.a; t < I.a + I.b; t++)
                    if (in.terms[t].src == ZXP_TERM_ONE)
                        for (int j = 0; j < 3; j++) c0[j] = gl_add(c0[j], in.terms[t].coef[j] % GL_P);
                align_kl(4);
                dot_k0[k] = o.kl.size();
                for (int j = 0; j < 3; j++) limbs3(c0[j]);
                first_use[k] = k;
                int64_t d_open = INT64_MIN;
                if (cost_stream) {
                    // only sources whose last read is this DOT count (others stay live anyway)
                    std::vector<std::pair<int64_t, int64_t>> cand;  // (definition, VGPRs freed)
                    for (uint32_t t = I.a; t < I.a + I.b; t++) {
                        const int64_t d = def_of(in.terms[t]);
                        if (d < 0 || last_read[in.terms[t].src] != (int64_t)k) continue;
                        cand.push_back({d, 2});  // per term: a base value or one component of an F_p^3 temporary
                    }
                    d_open = open_point(cand, k, three ? 18 : 6);
                }
                for (uint32_t t = I.a; t < I.a + I.b; t++) {
                    const zxp_term &tm = in.terms[t];
                    const int64_t d = def_of(tm);
                    if (d < 0) continue;  // not a temporary, or never written: the value is 0
                    if (cost_stream ? (d < d_open || last_read[tm.src] != (int64_t)k) : (int64_t)k - d > stream_span)
                        continue;  // read at the DOT instead
                    streamed_term[t] = 1;
                    stream[d].push_back(Stream{k, three, tmp_name(tm), limbs6x3(tm.coef)});
                    first_use[k] = std::min<uint32_t>(first_use[k], (uint32_t)d);
                }
            }
            if (D.kind == ZXP_TMP1) last1[D.a] = k;
            if (D.kind == ZXP_TMP3) last3[D.a] = k;
        }
        declare_at.resize(in.n_instr);
        for (uint32_t k = 0; k < in.n_instr; k++)
            if (first_use[k] != UINT32_MAX) declare_at[first_use[k]].push_back(k);
    }
    // cost mode: open the accumulators (A VGPRs) of DOT k at the definition
    // d_j that minimises A (k - d_j) + sum over the earlier-defined
    // sources w_i (k - d_i) (those wait in registers); INT64_MAX: no streaming
    static int64_t open_point(std::vector<std::pair<int64_t, int64_t>> &cand, int64_t k, int64_t A)
    {
        std::sort(cand.begin(), cand.end());
        int64_t wait = 0;  // sum w_i (k - d_i) over the sources before j
        for (const auto &c : cand) wait += c.second * (k - c.first);
        int64_t best = wait, acc = 0, d_open = INT64_MAX;
        for (size_t j = 0; j < cand.size(); j++) {
            const int64_t c = A * (k - cand[j].first) + acc;
            if (c < best) {
                best = c;
                d_open = cand[j].first;
            }
            acc += cand[j].second * (k - cand[j].first);
        }
        return d_open;
    }

    // ---- phase 5: emission.  Reads the plan; appends to body / dot_decls, kc, zt, kl (fused constants, terms not streamed)
    // a column read as text; 1: a cross-row read of a written column (interpreter)
    int col_read(uint32_t sec, uint32_t col, int32_t sh, std::string &e)
    {
        const uint32_t j = sl.slot(sec, col);
        if (sl.is_written(j)) {
            const int64_t w = sl.live_reg(j, sh);
            if (w >= 0) {
                e = "w" + std::to_string(w) + "_0";
                return 0;
            }
            if (sh != 0) return 1;
        }
        e.assign("C(", 2);
        app_num(e, j);
        e += ',';
        if (sh < 0) e += '-';
        app_num(e, (uint64_t)(sh < 0 ? -(int64_t)sh : sh));
        e += ",i_0)";
        return 0;
    }
    int operand(uint32_t idx, Expr &x)
    {
        const zxp_operand &p = in.opnd[idx];
        char b[160];
        switch (p.kind) {
        case ZXP_TMP1: x = {"a" + std::to_string(idx) + "_0", 1}; return 0;
        case ZXP_TMP3: x = {"b" + std::to_string(idx) + "_0", 3}; return 0;
        case ZXP_COL: x.dim = 1; return col_read(p.a, p.b, (int32_t)p.c, x.e);
        case ZXP_COL3: {
            std::string c0, c1, c2;
            if (col_read(p.a, p.b, (int32_t)p.c, c0) || col_read(p.a, p.b + 1, (int32_t)p.c, c1) ||
                col_read(p.a, p.b + 2, (int32_t)p.c, c2))
                return 1;
            x = {"gl3{{" + c0 + "," + c1 + "," + c2 + "}}", 3};
            return 0;
        }
        case ZXP_LIT: {
            const uint64_t v = ((uint64_t)p.a | ((uint64_t)p.b << 32)) % GL_P;
            snprintf(b, sizeof(b), "0x%llxULL", (unsigned long long)v);
            x = {b, 1};
            return 0;
        }
        case ZXP_PUB:
        case ZXP_CHAL:
        case ZXP_EVAL:
        case ZXP_IMM: {
            const uint64_t *v = p.kind == ZXP_PUB    ? in.publics + p.a
                                : p.kind == ZXP_CHAL ? in.challenges + 3 * p.a
                                : p.kind == ZXP_EVAL ? in.evals + 3 * p.a
                                                     : in.csts + 3 * p.a;
            const int dim = p.kind == ZXP_PUB ? 1 : p.kind == ZXP_IMM ? (int)p.b : 3;
            const size_t off = o.kc.size();
            for (int t = 0; t < dim; t++) o.kc.push_back(v[t] % GL_P);
            if (dim == 1)
                snprintf(b, sizeof(b), "p.kc[%zu]", off);
            else
                snprintf(b, sizeof(b), "gl3{{p.kc[%zu],p.kc[%zu],p.kc[%zu]}}", off, off + 1, off + 2);
            x = {b, dim};
            return 0;
        }
        case ZXP_X: uses_x = true; x = {"xv_0", 1}; return 0;
        case ZXP_XDIV: x = {"gl3{{gload(p.xdiv+3*i_0),gload(p.xdiv+3*i_0+1),gload(p.xdiv+3*i_0+2)}}", 3}; return 0;
        case ZXP_XDIVW: x = {"gl3{{gload(p.xdivw+3*i_0),gload(p.xdivw+3*i_0+1),gload(p.xdivw+3*i_0+2)}}", 3}; return 0;
        case ZXP_ZI: x = {"gload(p.zh + (i_0 & p.zmask))", 1}; return 0;
        default: return 1;
        }
    }
    // assignment of a value expression to a destination operand
    int assign(uint32_t didx, const Expr &r)
    {
        const zxp_operand &d = in.opnd[didx];
        const char *re = r.e.c_str(), *v0 = r.dim == 3 ? ".v[0]" : "";
        const uint32_t nc = d.kind == ZXP_COL3 ? 3 : d.kind == ZXP_COL ? 1 : 0;
        const bool scr = nc && d.a == ZXP_SEC_SCRATCH;
        if (scr || (nc && sl.store_now(d.a, d.b))) {
            // stored here: a carried value (scratch column), or a column the
            // program never reads, on row (i + shift) & m
            for (uint32_t c = 1; c < nc && !scr; c++)
                if (!sl.store_now(d.a, d.b + c)) return 1;  // mixed triple: keep the deferred form simple
            if (scr && d.c != 0) return 1;
            uint32_t j[3];  // (slots in column order: a slot is allocated where it is first asked for)
            for (uint32_t c = 0; c < nc; c++) j[c] = sl.slot(d.a, d.b + c);
            const std::string end = scr ? ", i_0)" : ", i_0, " + std::to_string((int32_t)d.c) + ")";
            auto st = [&](uint32_t c, const std::string &v) { return (scr ? "ZK_ST(" : "ZK_STS(") + std::to_string(j[c]) + ", " + v + end; };
            if (nc == 1)
                body += st(0, r.e + v0) + ";\n";
            else if (r.dim == 3)
                body += "{ const gl3 t_ = " + r.e + "; " + st(0, "t_.v[0]") + "; " + st(1, "t_.v[1]") + "; " + st(2, "t_.v[2]") + "; }\n";
            else
                body += st(0, r.e) + "; " + st(1, "0") + "; " + st(2, "0") + ";\n";
            return 0;
        }
        switch (d.kind) {
        case ZXP_TMP1:
        case ZXP_TMP3:  // (no printf: most lines of a body are these)
            body += d.kind == ZXP_TMP1 ? 'a' : 'b';
            app_num(body, didx);
            body += d.kind == ZXP_TMP3 && r.dim != 3 ? "_0 = gl3{{" : "_0 = ";
            body += r.e;
            body += d.kind == ZXP_TMP1 ? v0 : r.dim != 3 ? ", 0, 0}}" : "";
            body += ";\n";
            return 0;
        case ZXP_COL:
        case ZXP_COL3: {  // deferred: registers w<j>, stored at the end of the row
            uint32_t j[3];
            for (uint32_t c = 0; c < nc; c++) {
                j[c] = sl.wreg.at(std::make_pair(sl.slot(d.a, d.b + c), (int32_t)d.c));
                sl.wlive[j[c]] = 1;
            }
            if (nc == 1)
                appendf(body, "w%u_0 = %s%s;\n", j[0], re, v0);
            else if (r.dim == 3)
                appendf(body, "{ const gl3 t_ = %s; w%u_0 = t_.v[0]; w%u_0 = t_.v[1]; w%u_0 = t_.v[2]; }\n", re, j[0],
                        j[1], j[2]);
            else
                appendf(body, "w%u_0 = %s; w%u_0 = 0; w%u_0 = 0;\n", j[0], re, j[1], j[2]);
            return 0;
        }
        default: return 1;
        }
    }
    size_t kmap(size_t off, size_t n)  // n words of kl at off, in emission order
    {
        if (!split) return off;
        const size_t at = kl2.size();
        kl2.insert(kl2.end(), o.kl.begin() + off, o.kl.begin() + off + n);
        while (kl2.size() % 4) kl2.push_back(0);
        return at;
    }
    // DOT accumulators are initialised where the first term arrives
    void emit_declarations(uint32_t at)
    {
        for (uint32_t k : declare_at[at]) {
            const size_t k0 = dot_k0[k];
            if (in.ins[k].op == ZXP_DOT3) {
                appendf(dot_decls, "Dot3 D%u_0_0, D%u_1_0, D%u_2_0;\n", k, k, k);
                const size_t m0 = kmap(k0, 12);
                appendf(body, "D%u_0_0 = Dot3(K + %zu); D%u_1_0 = Dot3(K + %zu); D%u_2_0 = Dot3(K + %zu);\n", k, m0, k,
                        m0 + 4, k, m0 + 8);
            } else {
                appendf(dot_decls, "Dot3 D%u_0_0;\n", k);
                appendf(body, "D%u_0_0 = Dot3(K + %zu);\n", k, kmap(k0, 4));
            }
        }
    }
    void chunk_head()  // LDS base of this chunk; the next chunk's start patched in at the end (patch_chunks)
    {
        appendf(body, "const uint32_t *K = kbuf + %d - %zu; pf_ = kpre(p.kl, @KLO%zu@);\n",
                (int)(blk_no & 1) * JIT_KCHUNK, blk_lo, blk_no + 1);
    }
    // Compile time: LLVM's instruction selection and machine scheduler are
    // superlinear in basic-block size (a 600-instruction program took ~60 s
    // as one block).  Every `block` (1 KB) of source the body opens a
    // new block behind a uniform branch on an opaque 1 (zk_one(): an
    // s_mov_b32 the optimiser cannot see through, so it cannot merge the
    // blocks back), so each block is compiled on its own.  The block size also
    // bounds how far the scheduler hoists column loads: quarter-size
    // step42ns-shaped program at 2^24 rows, 256 / 512 / 1024 / 4096 bytes ->
    // 184 / 246 / 246 / 512+spills VGPRs, 453 / 359 / 303 / 394 ms, hiprtc
    // 63 / 56 / 80 / 116 s.
    // A limb chunk spans as many code blocks as its limbs fill (a workgroup
    // barrier every ~3-4 blocks; a chunk and barrier per block, the round-3
    // form, measured 43.3 against 45.4 Mrow/s on the zkEVM-sized quotient)
    // Source bytes of the body in the unit the block sizes were measured in: the row suffix _0 of a
    // name (NAMES, above) counts one byte; calls fall between statements: the body ends in a newline
    size_t body_bytes()
    {
        const char *b = body.data();
        const size_t end = body.size() < 2 ? 0 : body.size() - 2;
        for (; counted < end; counted++) suffixes += b[counted] == '_' && b[counted + 1] == '0' && !ident(b[counted + 2]);
        return body.size() - suffixes;
    }
    void maybe_split()
    {
        if (!split) return;
        const bool full = kl2.size() - blk_lo > JIT_KCHUNK - 256;
        if (body_bytes() - block_start < block && !full) return;
        if (full) {
            appendf(body, "kput(kbuf + %d, pf_);\n}\n__syncthreads();\n", (int)((blk_no + 1) & 1) * JIT_KCHUNK);
            blk_lo = kl2.size();
            blk_no++;
            klo_of.push_back(blk_lo);
            body += "if (zk_one()) {\n";
            chunk_head();
        } else {  // same chunk, new code block
            appendf(body, "}\nif (zk_one()) {\nconst uint32_t *K = kbuf + %d - %zu;\n", (int)(blk_no & 1) * JIT_KCHUNK,
                    blk_lo);
        }
        block_start = body_bytes();
    }
    void emit_streams(uint32_t at)
    {
        for (const Stream &st : stream[at]) {
            maybe_split();
            app_term(body, st.val, st.dot, kmap(st.kt, st.three ? 24 : 8), st.three);
        }
    }
    // the fused chains, where their first link stood
    int emit_fused()
    {
        const size_t G = ch.links.size();
        body += "{\n";
        for (size_t g = 0; g < G; g++) {
            align_kl(4);
            const size_t k0 = o.kl.size();
            for (int j = 0; j < 3; j++) limbs3(ch.konst[g][j]);
            appendf(body, "Dot3 F%zu_0_0 = Dot3(K + %zu), F%zu_1_0 = Dot3(K + %zu), F%zu_2_0 = Dot3(K + %zu);\n", g, k0, g,
                    k0 + 4, g, k0 + 8);
        }
        std::vector<uint32_t> fill(G, 0);  // terms since the chain's last reduction
        for (uint32_t mask = 1; mask < (1u << G); mask++) {
            std::vector<const FusedCol *> cols;
            for (const FusedCol &c : ch.cols)
                if (c.mask == mask) cols.push_back(&c);
            if (cols.empty()) continue;
            std::vector<int> mem;
            for (size_t g = 0; g < G; g++)
                if (mask >> g & 1) mem.push_back((int)g);
            const size_t R = mem.size();
            for (size_t p0 = 0; p0 < cols.size(); p0 += FUSE_PIECE) {
                const size_t n = std::min<size_t>(FUSE_PIECE, cols.size() - p0);
                const size_t np = (n + FUSE_U - 1) / FUSE_U * FUSE_U;
                const size_t off = o.zt.size();
                for (size_t e = 0; e < np; e++) {
                    const FusedCol &c = *cols[p0 + std::min(e, n - 1)];
                    for (size_t r = 0; r < R; r++) {
                        JitTerm jt;
                        memset(&jt, 0, sizeof(jt));
                        jt.ptr = o.cp[c.slot];
                        jt.sh = c.sh;
                        if (e < n)  // padding entries: zero limbs
                            for (int j = 0; j < 3; j++) zxp_limbs6(c.c[mem[r]][j] % GL_P, jt.c[j]);
                        o.zt.push_back(jt);
                    }
                }
                for (int g : mem)
                    if (fill[g] + np > 240) {  // Dot3 accumulators: reduce before 2^63 (gl_device.hpp)
                        appendf(body, "{ const uint64_t x0_ = F%d_0_0.fin(), x1_ = F%d_1_0.fin(), x2_ = F%d_2_0.fin(); "
                                      "F%d_0_0 = Dot3(); F%d_0_0.lane(x0_); F%d_1_0 = Dot3(); F%d_1_0.lane(x1_); "
                                      "F%d_2_0 = Dot3(); F%d_2_0.lane(x2_); }\n",
                                g, g, g, g, g, g, g, g, g);
                        fill[g] = 1;
                    }
                for (int g : mem) fill[g] += (uint32_t)np;
                appendf(body, "for (int q_ = 0; q_ < %zu; q_ += %zu) {\nconst JitTerm *t_ = ZT + %zu + (size_t)q_ * %zu;\n"
                              "uint64_t fv_0[%zu];\n", np, FUSE_U, off, R, FUSE_U);
                appendf(body, "_Pragma(\"unroll\") for (int u_ = 0; u_ < %zu; u_++) fv_0[u_] = gload(t_[u_ * %zu].ptr + "
                              "((i_0 + (uint64_t)t_[u_ * %zu].sh) & m));\n", FUSE_U, R, R);
                appendf(body, "_Pragma(\"unroll\") for (int u_ = 0; u_ < %zu; u_++) {\n", FUSE_U);
                for (size_t r = 0; r < R; r++)
                    appendf(body, "F%d_0_0.term(fv_0[u_], t_[u_ * %zu + %zu].c[0]); F%d_1_0.term(fv_0[u_], t_[u_ * %zu + %zu].c[1]); "
                                  "F%d_2_0.term(fv_0[u_], t_[u_ * %zu + %zu].c[2]);\n",
                            mem[r], R, r, mem[r], R, r, mem[r], R, r);
                body += "}\n}\n";
            }
        }
        for (size_t g = 0; g < G; g++) {
            char fin[128];
            snprintf(fin, sizeof(fin), "gl3{{F%zu_0_0.fin(), F%zu_1_0.fin(), F%zu_2_0.fin()}}", g, g, g);
            if (assign(in.ins[ch.links[g].back()].dst, Expr{fin, 3})) return 1;
        }
        body += "}\n";
        return 0;
    }
    int emit_dot(uint32_t k)
    {
        const zxp_instr &I = in.ins[k];
        const bool three = I.op == ZXP_DOT3;
        // column terms read from memory: looped from the term table when
        // there are many (code size, compile time), unrolled otherwise
        auto memcol = [&](const zxp_term &tm) {
            if (!col_term(in, tm)) return false;
            const zxp_operand &s = in.opnd[tm.src];
            return sl.live_reg(sl.slot(s.a, s.b), (int32_t)s.c) < 0;
        };
        uint32_t n_mem = 0;
        for (uint32_t t = I.a; t < I.a + I.b; t++) n_mem += memcol(in.terms[t]);
        // (large programs unroll every term: a looped DOT reads its
        // term records through vector loads, one wait each, and holds its
        // accumulators and in-flight loads across the loop -- the
        // zkEVM-sized quotient 1.27 s with loops, 0.57 s without)
        const bool loop = !split && n_mem >= in.dot_loop_min;
        if (loop) {
            const size_t t0 = o.zt.size();
            for (uint32_t t = I.a; t < I.a + I.b; t++) {
                const zxp_term &tm = in.terms[t];
                if (!memcol(tm)) continue;
                const zxp_operand &s = in.opnd[tm.src];
                if (sl.is_written(sl.slot(s.a, s.b)) && s.c != 0) return 1;
                JitTerm jt;
                memset(&jt, 0, sizeof(jt));
                jt.ptr = sl.ptr(s.a, s.b);
                jt.sh = (int64_t)(int32_t)s.c;
                for (int j = 0; j < 3; j++) zxp_limbs6(tm.coef[j] % GL_P, jt.c[j]);
                o.zt.push_back(jt);
            }
            if (three)
                appendf(body, "dot_cols<3>(D%u_0_0, D%u_1_0, D%u_2_0, ZT + %zu, %u, i_0, m);\n", k, k, k, t0, n_mem);
            else
                appendf(body, "dot_cols<1>(D%u_0_0, D%u_0_0, D%u_0_0, ZT + %zu, %u, i_0, m);\n", k, k, k, t0, n_mem);
        }
        for (uint32_t t = I.a; t < I.a + I.b; t++) {
            const zxp_term &tm = in.terms[t];
            if (tm.src == ZXP_TERM_ONE) continue;
            const zxp_operand &s = in.opnd[tm.src];
            std::string e;
            if (s.kind != ZXP_COL) {
                if (s.kind != ZXP_TMP1 && s.kind != ZXP_TMP3) return 1;
                if (streamed_term[t]) continue;  // accumulated at the temporary's definition
                maybe_split();
                e = tmp_name(tm);
            } else {
                if (loop && memcol(tm)) continue;
                maybe_split();
                if (col_read(s.a, s.b, (int32_t)s.c, e)) return 1;
            }
            app_term(body, e, k, kmap(limbs6x3(tm.coef), three ? 24 : 8), three);
        }
        char fin[128];
        if (three)
            snprintf(fin, sizeof(fin), "gl3{{D%u_0_0.fin(), D%u_1_0.fin(), D%u_2_0.fin()}}", k, k, k);
        else
            snprintf(fin, sizeof(fin), "D%u_0_0.fin()", k);
        return assign(I.dst, Expr{fin, three ? 3 : 1});
    }
    int emit_arith(uint32_t k)
    {
        const zxp_instr &I = in.ins[k];
        Expr A, B;
        if (operand(I.a, A)) return 1;
        if (I.op != ZXP_COPY && operand(I.b, B)) return 1;
        if (I.op == ZXP_COPY) return assign(I.dst, A);
        if (I.op != ZXP_MUL && I.op != ZXP_ADD && I.op != ZXP_SUB) return 1;
        const std::string nm = I.op == ZXP_MUL ? "mul" : I.op == ZXP_ADD ? "add" : "sub";
        // F_p^3 with F_p: the extension operand first (a - b3: gl3_rsub1(a, b3))
        std::string s;
        if (A.dim == 3 && B.dim == 3)
            s = "gl3_" + nm + "(" + A.e + ", " + B.e + ")";
        else if (A.dim == 3)
            s = "gl3_" + nm + "1(" + A.e + ", " + B.e + ")";
        else if (B.dim == 3)
            s = I.op == ZXP_SUB ? "gl3_rsub1(" + A.e + ", " + B.e + ")" : "gl3_" + nm + "1(" + B.e + ", " + A.e + ")";
        else
            s = "gl_" + nm + "(" + A.e + ", " + B.e + ")";
        return assign(I.dst, Expr{s, std::max(A.dim, B.dim)});
    }
    int emit_body()
    {
        // source bytes per block (segments: 512, round 6 -- paired with the
        // prefetch: without it the 512-byte segments ran 8 % slower)
        block = in.force_split ? (seg_ab().block ? seg_ab().block : 512) : 1024;
        body += split ? "if (zk_one()) {\n" : "{\n";
        if (split) {
            klo_of.push_back(0);
            chunk_head();
        }
        for (uint32_t k = 0; k < in.n_instr; k++) {
            const zxp_instr &I = in.ins[k];
            maybe_split();
            emit_declarations(k);
            if (ch.fused[k] >= 0) {
                if (k != ch.at) continue;
                if (emit_fused()) return 1;
            } else if (I.op == ZXP_DOT1 || I.op == ZXP_DOT3 ? emit_dot(k) : emit_arith(k)) {
                return 1;
            }
            emit_streams(k);
        }
        return 0;
    }

    // ---- phase 6 (split programs): the successors' chunk starts patched into the
    // body's @KLO<b>@ marks; kl becomes the table in emission order, padded for the last
    // copy.  1: a block's limbs overflow the LDS chunk (unsupported shape: the interpreter).
    int patch_chunks()
    {
        klo_of.push_back(kl2.size());
        for (size_t b = 0; b + 1 < klo_of.size(); b++)
            if (klo_of[b + 1] - klo_of[b] > (size_t)JIT_KCHUNK) return 1;
        std::string b2;
        b2.reserve(body.size());
        size_t pos = 0;
        for (;;) {
            const size_t at = body.find("@KLO", pos);
            if (at == std::string::npos) break;
            const size_t end = body.find('@', at + 4);
            b2.append(body, pos, at - pos);
            const size_t b = strtoull(body.c_str() + at + 4, nullptr, 10);
            b2 += std::to_string(b < klo_of.size() ? klo_of[b] : kl2.size());
            pos = end + 1;
        }
        b2.append(body, pos, std::string::npos);
        body.swap(b2);
        kl2.resize(kl2.size() + JIT_KCHUNK, 0);
        o.kl.swap(kl2);
        return 0;
    }

    // ---- phase 7: prelude, options, kernel head, declarations, body (after the text passes), deferred stores
    void assemble()
    {
        std::string &src = o.src;
        // Address space of the column pointers a split program reads (ZK_CP_AS; 0
        // generic = FLAT loads, 1 global = vector loads, 4 constant = scalar loads).
        // Block-split programs loaded every column pointer with a vector load ahead
        // of the dependent column load, and a limb table in global memory with FLAT
        // loads (its base sits behind an asm copy per block): quarter-size
        // step42ns-shaped program at 2^24 rows, limbs/pointers FLAT/vector 302 ms,
        // global/vector 272, FLAT/scalar 277, global/scalar 251, scalar/scalar 293
        // (scalar limbs: 106 SGPRs, spills) -- before the limbs moved to LDS chunks.
        // Small programs keep the compiler's choice.
        const bool klds = !split && jit_kl_lds(o.kl.size());
        src.clear();
        if (split) src += "#define ZK_CP_AS __attribute__((address_space(4)))\n";
        // (field add / sub keep their second correction as a select: with the
        // wave-uniform branch of gl_device.hpp ZK_RB the branches split the long
        // straight-line blocks, zkEVM-shaped quotient 39.9 -> 32.8 Mrow/s)
        // DOT limb reads (gl_device.hpp Dot3::term_al): explicit 16 + 8-byte loads for the
        // split programs' LDS chunks (-O1), the struct copy the -O2 vectorizer merges for the others
        if (!split) src += "#define ZK_LIMB_STRUCT 1\n";
        src += k_gl_device_src;
        appendf(src, "#define ZKJIT_KL_LDS %d\n", klds ? 1 : 0);
        appendf(src, "#define ZKJIT_SPLIT %d\n", split ? 1 : 0);
        appendf(src, "#define ZKJIT_KL_CHUNK %d\n", split ? JIT_KCHUNK : 0);  // large program: compile-time options (rtc_compile)
        // column terms per DOT-loop iteration (loads in flight; 8 / 16 measured neutral)
        src += "#define ZKJIT_UNROLL 4\n";
        if (in.waves_per_eu)
            appendf(src, "#define ZKJIT_WAVES __attribute__((amdgpu_waves_per_eu(%u)))\n", in.waves_per_eu);
        else
            src += "#define ZKJIT_WAVES\n";
        src += "#define ZKJIT_ROWS 1\n";
        // 32-bit column offsets from scalar bases (64-bit addresses, the round-3
        // form: 44.6 against 46.3 Mrow/s on the zkEVM-sized quotient)
        src += "#define ZKJIT_SADDR 1\n";
        // LDS column cache (lds_column_cache): block-split programs, 12
        // slots per lane and row (LDS: 2 KB per slot, row and workgroup; 16
        // slots measured +2 % on one box, -5 % on another)
        const SegAb &ab = seg_ab();
        const bool seg = split && in.force_split;  // a segment (zxp_segment)
        const uint32_t seg_w = in.waves_per_eu ? in.waves_per_eu : 4;
        const int lslots = seg ? (ab.waves ? (int)ab.slots : 16) : 12;
        // LDS budget of one workgroup (64 KB): the limb double buffer (kbuf)
        // or the whole limb table, then as many cache slots as still fit
        // (none: the uncached source)
        const size_t lds_limbs = split ? 2 * JIT_KCHUNK * 4 : (klds ? o.kl.size() * 4 : 0);
        const size_t slot_bytes = 256 * 8;
        const size_t lds_budget = seg ? 160 * 1024 / seg_w : 64 * 1024;
        const int fit = lds_limbs >= lds_budget ? 0 : (int)((lds_budget - lds_limbs) / slot_bytes);
        const int slots = std::min(lslots, fit);
        const bool lc = split && slots > 0 && lds_column_cache(body, slots) > 0;
        appendf(src, "#define ZKJIT_LCACHE %d\n", lc ? slots : 0);
        const uint32_t n_prefetch = seg ? prefetch_blocks(body, ab.waves ? ab.prefetch : 16, ab.dist ? ab.dist : 1) : 0;
        if (n_prefetch) src += "#define CSV(v, s, r) zk_cs(zkc_ + ((s) * ZKJIT_ROWS + (r)) * 256, (v))\n";
        src += k_kernel_head;
        src += "const uint64_t i_0 = ib_ + 0 * S_;\n";
        // Temporaries are named by SSA value (operand index), not by slot: the
        // code blocks sit behind branches the compiler cannot resolve, so a slot
        // variable reused through the program would keep every dead value it
        // held alive up to the slot's last read (the not-taken paths), i.e. all
        // slots live everywhere (~250 VGPRs on the zkEVM-sized quotient)
        std::vector<uint8_t> seen(in.n_opnd, 0);
        for (uint32_t k = 0; k < in.n_instr; k++) {
            const uint32_t d = in.ins[k].dst;
            if (d >= in.n_opnd || seen[d]) continue;
            seen[d] = 1;
            if (in.opnd[d].kind == ZXP_TMP1 || in.opnd[d].kind == ZXP_TMP3) {
                src += in.opnd[d].kind == ZXP_TMP1 ? "uint64_t a" : "gl3 b";
                app_num(src, d);
                src += "_0;\n";
            }
        }
        for (uint32_t r = 0; r < sl.wcell.size(); r++) appendf(src, "uint64_t w%u_0 = 0;\n", r);
        for (uint32_t r = 0; r < n_prefetch; r++) appendf(src, "uint64_t zpf%u_0;\n", r);
        if (uses_x)
            appendf(src, "const uint64_t ex__0 = i_0 << (%u - p.logomega);\n"
                         "const uint64_t xv_0 = gl_mul(p.x_start, gl_mul(gload(p.tw_lo + (ex__0 & %lluULL)), gload(p.tw_hi + (ex__0 >> %u))));\n",
                    TW_MAX_LOG, (unsigned long long)(TW_LEVEL_SIZE - 1), TW_LEVEL_BITS);
        src += dot_decls;
        src += body;
        src += "}\n";
        if (split) src += "if (live_) {\n";
        for (uint32_t r = 0; r < sl.wcell.size(); r++) {
            if (sl.wcell[r].second == 0)
                appendf(src, "gstore(const_cast<uint64_t *>(p.cp[%u]) + i_0, gl_canon(w%u_0));\n", sl.wcell[r].first, r);
            else
                appendf(src, "gstore(const_cast<uint64_t *>(p.cp[%u]) + ((i_0 + (uint64_t)(%d)) & m), gl_canon(w%u_0));\n",
                        sl.wcell[r].first, sl.wcell[r].second, r);
        }
        if (split) src += "}\n";
        src += "#undef C\n}\n";
    }
};

}  // namespace

int zxp_jit_build_source(const ZxpJitIn &in, ZxpJitSource &out)
{
    out = ZxpJitSource();
    Generator g(in, out);
    out.split = g.split;
    g.ch.fused.assign(in.n_instr, -1);
    if (!g.split) {  // (block-split programs fuse no chains)
        g.ch = detect_chains(in, g.sl);
        unroll_chains(in, g.sl, g.ch);
    }
    g.plan_dots();
    if (g.emit_body()) return 1;
    if (g.split && g.patch_chunks()) return 1;
    g.assemble();
    return 0;
}

}  // namespace zk
