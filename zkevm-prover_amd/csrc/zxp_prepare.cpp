// Host side of an expression-program evaluation (csrc/zxp_prepare.hpp):
// validate, plan, interpreter records.  No GPU, no HIP.
#include "zxp_prepare.hpp"

#include <algorithm>
#include <cstdlib>

#include "zxp_jit_source.hpp"  // zxp_limbs6, the host field (gl_host.hpp)

namespace zk {

int set_error(int code, const char *fmt, ...);  // api.hip

// no out-of-range reads in the kernels: every index and pointer they take
// from the program is checked here
int zxp_validate(const ZxpArgs &a)
{
    if (a.log_omega > TW_MAX_LOG || a.log_dom > a.log_omega) return set_error(ZKGPU_ERR_ARG, "zxp: domain too large");
    if (a.extend_bits > a.log_omega) return set_error(ZKGPU_ERR_ARG, "zxp: extend bits exceed the domain");
    for (uint32_t k = 0; k < a.n_instr; k++) {
        const zxp_instr &I = a.instr[k];
        if (I.dst >= a.n_opnd || I.a >= a.n_opnd || (I.op != ZXP_COPY && I.b >= a.n_opnd) || I.op > 3)
            return set_error(ZKGPU_ERR_ARG, "zxp: instruction %u out of range", k);
    }
    const zkgpu_sections &S = *a.sections;
    // a row list: the rows read are rows of the whole section, the rows stored are the list's
    // places, so a section is one or the other, and what is stored to is n_rows long
    bool stored[SEC_COUNT] = {};
    if (a.row_list) {
        if (!a.rows) return set_error(ZKGPU_ERR_ARG, "zxp rows: null row list");
        if (a.n_rows > ZXP_MAX_LIST_ROWS)
            return set_error(ZKGPU_ERR_ARG, "zxp rows: %u rows exceed %u", a.n_rows, ZXP_MAX_LIST_ROWS);
        bool read[SEC_COUNT] = {};
        const auto col = [&](uint32_t k) {
            const zxp_operand &o = a.opnd[k];
            return (o.kind == ZXP_COL || o.kind == ZXP_COL3) && o.a < SEC_COUNT;
        };
        for (uint32_t k = 0; k < a.n_instr; k++) {
            const zxp_instr &I = a.instr[k];
            if (col(I.a)) read[a.opnd[I.a].a] = true;
            if (I.op != ZXP_COPY && col(I.b)) read[a.opnd[I.b].a] = true;
            if (col(I.dst)) {
                if (a.opnd[I.dst].c)
                    return set_error(ZKGPU_ERR_ARG, "zxp rows: instruction %u stores at row shift %d", k,
                                     (int)(int32_t)a.opnd[I.dst].c);
                stored[a.opnd[I.dst].a] = true;
            }
        }
        for (uint32_t s = 0; s < SEC_COUNT; s++)
            if (read[s] && stored[s])
                return set_error(ZKGPU_ERR_ARG, "zxp rows: section %u is both read and stored to", s);
        for (uint32_t s = 0; s < SEC_COUNT; s++)
            if (stored[s] && S.ld[s] < a.n_rows)
                return set_error(ZKGPU_ERR_ARG, "zxp rows: section %u is stored to and holds %llu rows, not %u", s,
                                 (unsigned long long)S.ld[s], a.n_rows);
    }
    for (uint32_t k = 0; k < a.n_opnd; k++) {
        const zxp_operand &o = a.opnd[k];
        bool bad = false;
        switch (o.kind) {
        case ZXP_TMP1: bad = o.a >= a.n_tmp1; break;
        case ZXP_TMP3: bad = o.a >= a.n_tmp3; break;
        case ZXP_COL:
        case ZXP_COL3: {
            const uint32_t w = o.kind == ZXP_COL3 ? 3 : 1;
            const int32_t sh = (int32_t)o.c;
            // without wrap-around a shifted read touches halo rows [2^log_dom, 2^log_dom + sh); a shifted
            // store (the reference's parser opcodes 101-114 / 119 write pols[off + ((i + s) % N) * stride],
            // step3.parser.cpp) lands on row (i + s) mod 2^log_dom, in a row block on local row i + s, the
            // last s of them in the halo rows, which the caller hands to the next block's owner
            const uint64_t need = o.a < SEC_COUNT && stored[o.a]
                                      ? a.n_rows
                                      : (1ULL << a.log_dom) + (a.wrap ? 0 : (uint64_t)(sh > 0 ? sh : 0));
            bad = o.a >= SEC_COUNT || !S.sec[o.a] || (uint64_t)o.b + w > S.ncols[o.a] || S.ld[o.a] < need ||
                  (!a.wrap && sh < 0);
            break;
        }
        case ZXP_CHAL: bad = o.a >= 8; break;
        case ZXP_PUB: bad = o.a >= a.n_publics; break;
        case ZXP_EVAL: bad = o.a >= a.n_evals; break;
        case ZXP_XDIV: bad = !a.xdiv; break;
        case ZXP_XDIVW: bad = !a.xdivw; break;
        case ZXP_LIT:
        case ZXP_X:
        case ZXP_ZI: break;
        default: bad = true;
        }
        if (bad) return set_error(ZKGPU_ERR_ARG, "zxp: operand %u (kind %u) invalid", k, o.kind);
    }
    if (a.extend_bits > 6) return set_error(ZKGPU_ERR_ARG, "zxp: extend bits > 6");
    // (the kernels keep a column's stride in 32 bits)
    for (uint32_t k = 0; k < a.n_opnd; k++)
        if ((a.opnd[k].kind == ZXP_COL || a.opnd[k].kind == ZXP_COL3) && S.ld[a.opnd[k].a] > 0xFFFFFFFFULL)
            return set_error(ZKGPU_ERR_ARG, "zxp: section %u stride exceeds 2^32", a.opnd[k].a);
    return 0;
}

// Temp-slot allocation for a ZXP program.  Program producers (the synthetic
// builder, a chelpers converter) may give every intermediate its own temp;
// the LDS footprint per workgroup is (slots x 64 rows x 8 B), which bounds
// occupancy.  Each temp identity lives over [first occurrence, last
// occurrence]; a linear scan packs the intervals of each pool (base / ext)
// into the fewest slots.  An interval may start at the instruction where
// another ends: the interpreter loads both sources before it stores the
// destination.  The operand table is rewritten (duplicates are harmless).
static void zxp_alloc_slots(const zxp_instr *in, uint32_t n_instr, std::vector<zxp_operand> &op, uint32_t &n_tmp1,
                            uint32_t &n_tmp3)
{
    for (int pool = 0; pool < 2; pool++) {
        const uint32_t kind = pool ? ZXP_TMP3 : ZXP_TMP1;
        const uint32_t n_id = pool ? n_tmp3 : n_tmp1;
        std::vector<uint32_t> first(n_id, UINT32_MAX), last(n_id, 0);
        for (uint32_t k = 0; k < n_instr; k++) {
            const uint32_t refs[3] = {in[k].dst, in[k].a, in[k].op == ZXP_COPY ? in[k].a : in[k].b};
            for (uint32_t r : refs)
                if (op[r].kind == kind) {
                    const uint32_t id = op[r].a;
                    first[id] = std::min(first[id], k);
                    last[id] = std::max(last[id], k);
                }
        }
        std::vector<uint32_t> order;
        for (uint32_t id = 0; id < n_id; id++)
            if (first[id] != UINT32_MAX) order.push_back(id);
        std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return first[x] < first[y]; });
        std::vector<uint32_t> slot_of(n_id, 0), slot_end;
        for (uint32_t id : order) {
            uint32_t s = 0;
            while (s < slot_end.size() && slot_end[s] > first[id]) s++;
            if (s == slot_end.size()) slot_end.push_back(0);
            slot_end[s] = last[id];
            slot_of[id] = s;
        }
        for (auto &o : op)
            if (o.kind == kind) o.a = slot_of[o.a];
        const uint32_t used = (uint32_t)std::max<size_t>(slot_end.size(), 1);
        (pool ? n_tmp3 : n_tmp1) = used;
    }
}

// what both kernels take for granted of the program they run
static int check_program(const zxp_compiled &c)
{
    for (uint32_t k = 0; k < c.n_instr; k++) {
        const zxp_instr &I = c.instr[k];
        if (I.op == ZXP_DOT1 || I.op == ZXP_DOT3)
            for (uint32_t t = I.a; t < I.a + I.b; t++) {
                if (c.term[t].src == ZXP_TERM_ONE) continue;
                const uint32_t kind = c.opnd[c.term[t].src].kind;
                if (kind != ZXP_COL && kind != ZXP_TMP1 && kind != ZXP_TMP3)
                    return set_error(ZKGPU_ERR_ARG, "zxp: DOT term source kind %u", kind);
            }
        const uint32_t dk = c.opnd[I.dst].kind;
        if (dk != ZXP_TMP1 && dk != ZXP_TMP3 && dk != ZXP_COL && dk != ZXP_COL3)
            return set_error(ZKGPU_ERR_ARG, "zxp: instruction %u writes a read-only operand", k);
    }
    return 0;
}

int zxp_plan(const ZxpArgs &a, ZxpPlan &p)
{
    // compile (csrc/zxp_compile.cpp): linear-combination fusion + SSA slots.
    // ZKGPU_ZXP_FUSE=0 runs the source program as is (slot packing only).
    const char *env_fuse = getenv("ZKGPU_ZXP_FUSE");
    const char *env_terms = getenv("ZKGPU_ZXP_MAX_TERMS");
    const int fuse = env_fuse ? atoi(env_fuse) : 1;
    const uint32_t max_terms = env_terms ? (uint32_t)atoi(env_terms) : 0u;
    // The compiled program runs as a run-time compiled straight-line kernel
    // (csrc/zxp_jit.hip, compiled once per program per process) on domains of
    // 2^16 rows and more, where it pays for its ~1-2 s compile; smaller
    // domains use the interpreter.  ZKGPU_ZXP_JIT=0 never, =2 always.
    const char *env_jit = getenv("ZKGPU_ZXP_JIT");
    const int jit_mode = env_jit ? atoi(env_jit) : 1;
    // (the compiled kernels address a column with a 32-bit byte offset:
    // domains up to 2^28 rows plus their halo)
    // (a row list always runs on the interpreter: at most 4096 rows)
    p.jit = !a.row_list && fuse && a.log_dom <= 28 && (jit_mode == 2 || (jit_mode == 1 && a.log_dom >= 16));
    int rc;
    if (fuse) {
        // (one compile serves both paths: measured, longer DOTs / fused DOT
        // column passes / no live-temporary cap made the compiled kernels slower)
        if ((rc = zkgpu_zxp_compile(a.instr, a.n_instr, a.opnd, a.n_opnd, a.n_tmp1, a.n_tmp3, a.challenges, a.publics,
                                    a.n_publics, a.evals, a.n_evals, max_terms, &p.prog)))
            return rc;
    } else {
        p.packed.assign(a.opnd, a.opnd + a.n_opnd);
        uint32_t n_tmp1 = a.n_tmp1, n_tmp3 = a.n_tmp3;
        zxp_alloc_slots(a.instr, a.n_instr, p.packed, n_tmp1, n_tmp3);
        p.prog = zxp_compiled{a.instr, a.n_instr, p.packed.data(), a.n_opnd, nullptr, 0, nullptr, 0, n_tmp1, n_tmp3};
    }
    if ((rc = check_program(p.prog))) return rc;
    p.n_dot_terms = 0;
    for (uint32_t t = 0; t < p.prog.n_term; t++) p.n_dot_terms += p.prog.term[t].src != ZXP_TERM_ONE;
    // zhInv[j] = 1/(7^N * W[eb]^j - 1)  (zhInv.cpp:7-31), N = 2^(log_omega - eb); only for a program
    // with a ZI operand (on a domain where Z_H vanishes -- the trace domain, x_start 1 -- it has no
    // inverse, and no program without ZI reads the table: it stays zero)
    p.n_zhinv = 1u << a.extend_bits;
    p.uses_zi = false;
    for (uint32_t k = 0; k < a.n_opnd; k++) p.uses_zi |= a.opnd[k].kind == ZXP_ZI;
    const uint64_t sn = h_pow(7, 1ULL << (a.log_omega - a.extend_bits)), we = h_w(a.extend_bits);
    uint64_t w = 1;
    for (uint32_t j = 0; j < p.n_zhinv; j++) {
        const uint64_t x = h_mul(sn, w);  // < HP
        p.zhinv[j] = p.uses_zi ? h_inv(x ? x - 1 : HP - 1) : 0;
        w = h_mul(w, we);
    }
    p.bytes = 0;
    for (uint32_t k = 0; k < a.n_opnd; k++) {
        const uint32_t kind = a.opnd[k].kind;
        p.bytes += kind == ZXP_COL ? 1 : (kind == ZXP_COL3 || kind == ZXP_XDIV || kind == ZXP_XDIVW) ? 3 : 0;
    }
    p.bytes *= 8.0 * (a.row_list ? (double)a.n_rows : (double)(1ULL << a.log_dom));
    return 0;
}

namespace {

// resolves operands to (kind, pointer, shift / slot, stride, immediate)
struct Decoder {
    const ZxpArgs &a;
    const ZxpPlan &p;
    const uint64_t *zh_dev;

    const uint64_t *column(const zxp_operand &o) const
    {
        return a.sections->sec[o.a] + (uint64_t)o.b * a.sections->ld[o.a];
    }
    int32_t slot1(uint32_t s) const { return (int32_t)(s * 64); }
    int32_t slot3(uint32_t s, uint32_t comp) const { return (int32_t)((p.prog.n_tmp1 + 3 * s + comp) * 64); }

    void operator()(const zxp_operand &o, uint32_t &kind, const uint64_t *&ptr, int32_t &ii, uint32_t &ld,
                    uint64_t *imm) const
    {
        ptr = nullptr;
        ii = 0;
        ld = 0;
        imm[0] = imm[1] = imm[2] = 0;
        switch (o.kind) {
        case ZXP_TMP1: kind = DK_T1; ii = slot1(o.a); break;
        case ZXP_TMP3: kind = DK_T3; ii = slot3(o.a, 0); break;
        case ZXP_COL:
        case ZXP_COL3:
            kind = o.kind == ZXP_COL ? DK_C1 : DK_C3;
            ptr = column(o);
            ii = (int32_t)o.c;
            ld = (uint32_t)a.sections->ld[o.a];
            break;
        case ZXP_LIT: kind = DK_IMM1; imm[0] = ((uint64_t)o.a | ((uint64_t)o.b << 32)) % HP; break;
        case ZXP_PUB: kind = DK_IMM1; imm[0] = a.publics[o.a] % HP; break;
        case ZXP_CHAL:
            kind = DK_IMM3;
            for (int t = 0; t < 3; t++) imm[t] = a.challenges[3 * o.a + t] % HP;
            break;
        case ZXP_EVAL:
            kind = DK_IMM3;
            for (int t = 0; t < 3; t++) imm[t] = a.evals[3 * o.a + t] % HP;
            break;
        case ZXP_IMM:
            kind = o.b == 3 ? DK_IMM3 : DK_IMM1;
            for (int t = 0; t < 3; t++) imm[t] = p.prog.cst[3 * o.a + t];
            break;
        case ZXP_X: kind = DK_X; break;
        case ZXP_XDIV: kind = DK_I3; ptr = a.xdiv; break;
        case ZXP_XDIVW: kind = DK_I3; ptr = a.xdivw; break;
        case ZXP_ZI: kind = DK_ZI; ptr = zh_dev; ii = (int32_t)(p.n_zhinv - 1); break;
        default: kind = DK_IMM1; break;
        }
    }
};

}  // namespace

int zxp_records(const ZxpArgs &a, const ZxpPlan &p, const uint64_t *zh_dev, std::vector<ZOp> &ops,
                std::vector<ZTerm> &terms)
{
    const zxp_compiled &c = p.prog;
    const uint64_t slots = (uint64_t)c.n_tmp1 + 3ULL * c.n_tmp3;
    if (slots * 64 * 8 > 160 * 1024)
        return set_error(ZKGPU_ERR_ARG, "zxp: %llu temp slots exceed LDS", (unsigned long long)slots);
    const Decoder decode{a, p, zh_dev};
    ops.assign(c.n_instr, ZOp{});  // (zero: the padding is uploaded too)
    terms.clear();
    terms.reserve(p.n_dot_terms);
    for (uint32_t k = 0; k < c.n_instr; k++) {
        const zxp_instr &I = c.instr[k];
        ZOp &z = ops[k];
        z.op = I.op;
        if (z.op == ZXP_DOT1 || z.op == ZXP_DOT3) {
            uint64_t c0[3] = {0, 0, 0};
            z.ia = (int32_t)terms.size();
            for (uint32_t t = I.a; t < I.a + I.b; t++) {
                const zxp_term &tm = c.term[t];
                if (tm.src == ZXP_TERM_ONE) {
                    for (int j = 0; j < 3; j++) c0[j] = h_add(c0[j], tm.coef[j] % HP);
                    continue;
                }
                ZTerm zt{};
                const zxp_operand &o = c.opnd[tm.src];  // COL, TMP1 or TMP3 (check_program)
                if (o.kind == ZXP_COL) {
                    zt.kind = DK_C1;
                    zt.ptr = decode.column(o);
                    zt.ii = (int32_t)o.c;
                } else {
                    zt.kind = DK_T1;
                    zt.ii = o.kind == ZXP_TMP1 ? decode.slot1(o.a) : decode.slot3(o.a, tm.comp);
                }
                for (int j = 0; j < 3; j++) zxp_limbs6(tm.coef[j] % HP, zt.c[j]);
                terms.push_back(zt);
            }
            z.ib = (int32_t)(terms.size() - (size_t)z.ia);
            uint32_t *kl = reinterpret_cast<uint32_t *>(z.ima);  // 9 u32 over ima/imb
            for (int j = 0; j < 3; j++) {
                kl[3 * j] = (uint32_t)(c0[j] & ((1u << 22) - 1));
                kl[3 * j + 1] = (uint32_t)((c0[j] >> 22) & ((1u << 21) - 1));
                kl[3 * j + 2] = (uint32_t)(c0[j] >> 43);
            }
        } else {
            decode(c.opnd[I.a], z.ka, z.pa, z.ia, z.lda, z.ima);
            if (I.op != ZXP_COPY) decode(c.opnd[I.b], z.kb, z.pb, z.ib, z.ldb, z.imb);
        }
        const uint64_t *pd;
        uint64_t dimm[3];
        decode(c.opnd[I.dst], z.kd, pd, z.id, z.ldd, dimm);  // a temp or a column (check_program)
        z.pd = const_cast<uint64_t *>(pd);
    }
    return 0;
}

}  // namespace zk
