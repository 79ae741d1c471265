// Stand-alone run of the host side of an expression evaluation
// (csrc/zxp_prepare.cpp: validate, plan, interpreter records) with the
// library's other host-only sources, so it runs under the host sanitizers
// with nothing loaded into Python (tests/test_cpp_zxp_prepare.py).
//
// usage: zxp_prepare_check CASE.bin [OUT.bin]
// CASE.bin (u64 words): magic, n_instr, n_opnd, n_tmp1, n_tmp3, n_publics,
// n_evals, log_dom, log_omega, wrap, extend_bits, x_start, xdiv (0 null, 1
// data follows, else a placeholder address), xdivw (same), 12 sections of
// (sec, ld, ncols) with sec 0 null, 1 data follows, else a placeholder
// address; then instr and opnd (u32 x 4 each), 24 challenge words, the
// publics, 3 n_evals eval words; then the data of every section with sec = 1
// (column-major, ld ncols words), of xdiv and of xdivw (3 2^log_dom words).
// ZKGPU_ZXP_FUSE / _MAX_TERMS / _JIT are read from the environment as the
// library reads them.
//
// Runs validate and plan.  An error prints "error <code>: <message>" and ends
// the run with status 0.  Otherwise, with OUT.bin: on the compiled path the
// source generator must leave the program to the interpreter (prints "jit:
// unsupported program shape"), which takes the same plan; the records are
// built over sections allocated at their exact size, checked (immediates and
// coefficients below p, column pointers inside their section) and replayed
// row by row, instruction by instruction -- the oracle's order -- in plain
// 128-bit modular arithmetic; the sections with data are written to OUT.bin
// in index order.  The replay is test code: the library has no host evaluator.
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../zkevm-prover_amd/csrc/zxp_jit_source.hpp"
#include "../../zkevm-prover_amd/csrc/zxp_prepare.hpp"

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

using namespace zk;
typedef unsigned __int128 u128;

static const uint64_t P = 0xFFFFFFFF00000001ULL;
static uint64_t add(uint64_t a, uint64_t b) { return (uint64_t)(((u128)a + b) % P); }
static uint64_t sub(uint64_t a, uint64_t b) { return (uint64_t)(((u128)a + P - b % P) % P); }
static uint64_t mul(uint64_t a, uint64_t b) { return (uint64_t)((u128)a * b % P); }

struct V3 {
    uint64_t v[3];
    int dim;
};
// F_p^3 = F_p[x] / (x^3 - x - 1)
static V3 mul3(const V3 &a, const V3 &b)
{
    const uint64_t c0 = mul(a.v[0], b.v[0]), c1 = add(mul(a.v[0], b.v[1]), mul(a.v[1], b.v[0])),
                   c2 = add(add(mul(a.v[0], b.v[2]), mul(a.v[1], b.v[1])), mul(a.v[2], b.v[0])),
                   c3 = add(mul(a.v[1], b.v[2]), mul(a.v[2], b.v[1])), c4 = mul(a.v[2], b.v[2]);
    // x^3 = x + 1, x^4 = x^2 + x
    return V3{{add(c0, c3), add(add(c1, c3), c4), add(c2, c4)}, 3};
}

static int fail(const char *what)
{
    fprintf(stderr, "zxp_prepare_check: %s\n", what);
    return 2;
}

static uint64_t limbs3(const uint32_t *l) { return (uint64_t)l[0] + ((uint64_t)l[1] << 22) + ((uint64_t)l[2] << 43); }

struct Replay {
    const ZxpArgs &a;
    const ZxpPlan &p;
    const std::vector<ZOp> &ops;
    const std::vector<ZTerm> &terms;
    std::vector<uint64_t> lds;  // slot s of lane l at lds[s * 64 + l], as in the kernel
    std::vector<uint64_t> x;
    uint64_t rmask;

    V3 load(uint32_t kind, const uint64_t *ptr, int32_t ii, uint32_t ld, const uint64_t *imm, uint64_t i) const
    {
        const int lane = (int)(i & 63);
        V3 r{{0, 0, 0}, 1};
        switch (kind) {
        case DK_T1: r.v[0] = lds[ii + lane]; break;
        case DK_T3: r = V3{{lds[ii + lane], lds[ii + 64 + lane], lds[ii + 128 + lane]}, 3}; break;
        case DK_C1: r.v[0] = ptr[(i + (uint64_t)(int64_t)ii) & rmask]; break;
        case DK_C3: {
            const uint64_t *q = ptr + ((i + (uint64_t)(int64_t)ii) & rmask);
            r = V3{{q[0], q[ld], q[2 * (uint64_t)ld]}, 3};
            break;
        }
        case DK_IMM1: r.v[0] = imm[0]; break;
        case DK_IMM3: r = V3{{imm[0], imm[1], imm[2]}, 3}; break;
        case DK_X: r.v[0] = x[i]; break;
        case DK_I3: r = V3{{ptr[3 * i], ptr[3 * i + 1], ptr[3 * i + 2]}, 3}; break;
        case DK_ZI: r.v[0] = ptr[i & (uint32_t)ii]; break;
        default: break;
        }
        return r;
    }

    void row(uint64_t i)
    {
        const int lane = (int)(i & 63);
        std::fill(lds.begin(), lds.end(), 0);  // (the oracle's rows start with zero temporaries)
        for (const ZOp &z : ops) {
            V3 r{{0, 0, 0}, 1};
            if (z.op >= ZXP_DOT1) {
                const uint32_t *k0 = reinterpret_cast<const uint32_t *>(z.ima);
                const int nc = z.op == ZXP_DOT3 ? 3 : 1;
                r.dim = nc;
                for (int j = 0; j < nc; j++) r.v[j] = limbs3(k0 + 3 * j);
                for (int t = 0; t < z.ib; t++) {
                    const ZTerm &tt = terms[z.ia + t];
                    const uint64_t s =
                        tt.kind == DK_T1 ? lds[tt.ii + lane] : tt.ptr[(i + (uint64_t)(int64_t)tt.ii) & rmask];
                    for (int j = 0; j < nc; j++) r.v[j] = add(r.v[j], mul(limbs3(tt.c[j]), s));
                }
            } else {
                const V3 va = load(z.ka, z.pa, z.ia, z.lda, z.ima, i);
                if (z.op == ZXP_COPY) {
                    r = va;
                } else {
                    const V3 vb = load(z.kb, z.pb, z.ib, z.ldb, z.imb, i);
                    r.dim = (va.dim == 3 || vb.dim == 3) ? 3 : 1;
                    if (z.op == ZXP_MUL) {
                        if (va.dim == 3 && vb.dim == 3)
                            r = mul3(va, vb);
                        else {
                            const V3 &e = va.dim == 3 ? va : vb;
                            const uint64_t s = va.dim == 3 ? vb.v[0] : va.v[0];
                            for (int j = 0; j < r.dim; j++) r.v[j] = mul(e.v[j], s);
                        }
                    } else {  // a base operand carries zeros in components 1, 2
                        for (int j = 0; j < r.dim; j++)
                            r.v[j] = z.op == ZXP_ADD ? add(va.v[j], vb.v[j]) : sub(va.v[j], vb.v[j]);
                    }
                }
            }
            const uint64_t hi[2] = {r.dim == 3 ? r.v[1] : 0, r.dim == 3 ? r.v[2] : 0};
            switch (z.kd) {
            case DK_T1: lds[z.id + lane] = r.v[0]; break;
            case DK_T3:
                lds[z.id + lane] = r.v[0];
                lds[z.id + 64 + lane] = hi[0];
                lds[z.id + 128 + lane] = hi[1];
                break;
            case DK_C1:
            case DK_C3: {
                uint64_t *q = z.pd + ((i + (uint64_t)(int64_t)z.id) & rmask);
                q[0] = r.v[0] % P;
                if (z.kd == DK_C3) {
                    q[z.ldd] = hi[0] % P;
                    q[2 * (uint64_t)z.ldd] = hi[1] % P;
                }
                break;
            }
            default: break;
            }
        }
    }
};

int main(int argc, char **argv)
{
    if (argc != 2 && argc != 3) return fail("usage: zxp_prepare_check CASE.bin [OUT.bin]");
    std::vector<uint64_t> w;
    {
        FILE *f = fopen(argv[1], "rb");
        if (!f) return fail("cannot open the case");
        uint64_t buf[4096];
        for (size_t n; (n = fread(buf, 8, 4096, f)) > 0;) w.insert(w.end(), buf, buf + n);
        fclose(f);
    }
    const size_t o_instr = 14 + 3 * 12;
    if (w.size() < o_instr || w[0] != 0x5a5850505245ULL) return fail("bad header");
    ZxpArgs a;
    a.n_instr = (uint32_t)w[1], a.n_opnd = (uint32_t)w[2], a.n_tmp1 = (uint32_t)w[3], a.n_tmp3 = (uint32_t)w[4];
    a.n_publics = (uint32_t)w[5], a.n_evals = (uint32_t)w[6];
    a.log_dom = (uint32_t)w[7], a.log_omega = (uint32_t)w[8], a.wrap = (int)w[9], a.extend_bits = (uint32_t)w[10];
    a.x_start = w[11];
    const size_t o_opnd = o_instr + 2 * (size_t)a.n_instr, o_ch = o_opnd + 2 * (size_t)a.n_opnd, o_pub = o_ch + 24,
                 o_ev = o_pub + a.n_publics, o_data = o_ev + 3 * (size_t)a.n_evals;
    if (w.size() < o_data) return fail("bad length");
    // exact-size copies of every table, so a read past one's end is seen
    const std::vector<uint64_t> instr(w.begin() + o_instr, w.begin() + o_opnd), opnd(w.begin() + o_opnd, w.begin() + o_ch),
        chal(w.begin() + o_ch, w.begin() + o_pub), pub(w.begin() + o_pub, w.begin() + o_ev),
        ev(w.begin() + o_ev, w.begin() + o_data);
    a.instr = (const zxp_instr *)instr.data();
    a.opnd = (const zxp_operand *)opnd.data();
    a.challenges = chal.data();
    a.publics = pub.data();
    a.evals = ev.data();
    size_t at = o_data;
    std::vector<std::unique_ptr<uint64_t[]>> owned;
    auto table = [&](uint64_t how, size_t words) -> uint64_t * {
        if (how != 1) return (uint64_t *)(uintptr_t)how;  // null, or a placeholder never dereferenced
        if (w.size() < at + words) return nullptr;
        owned.emplace_back(new uint64_t[words ? words : 1]);
        memcpy(owned.back().get(), w.data() + at, words * 8);
        at += words;
        return owned.back().get();
    };
    zkgpu_sections S;
    size_t sec_words[12];
    for (int k = 0; k < 12; k++) {
        const uint64_t *h = &w[14 + 3 * k];
        S.ld[k] = h[1];
        S.ncols[k] = (uint32_t)h[2];
        sec_words[k] = h[0] == 1 ? (size_t)(h[1] * h[2]) : 0;
        S.sec[k] = table(h[0], sec_words[k]);
        if (h[0] == 1 && !S.sec[k]) return fail("bad length (sections)");
    }
    a.sections = &S;
    const size_t dom = (size_t)1 << (a.log_dom < 32 ? a.log_dom : 0);
    a.xdiv = table(w[12], 3 * dom);
    a.xdivw = table(w[13], 3 * dom);
    if ((w[12] == 1 && !a.xdiv) || (w[13] == 1 && !a.xdivw) || at != w.size()) return fail("bad length (data)");

    int rc;
    ZxpPlan plan;
    if ((rc = zxp_validate(a)) || (rc = zxp_plan(a, plan))) {
        printf("error %d: %s\n", rc, g_msg);
        return 0;
    }
    if (argc == 2) {
        puts(plan.jit ? "planned: compiled kernels" : "planned: interpreter");
        return 0;
    }
    if (plan.jit) {  // as zkgpu_zxp_eval_dev: the interpreter only where the generator declines
        ZxpJitSource src;
        const ZxpJitIn J = zxp_jit_in(plan.prog, a.sections, a.challenges, a.publics, a.evals);
        if (zxp_jit_build_source(J, src) != 1) return fail("the compiled kernels run this program: nothing to replay");
        puts("jit: unsupported program shape");
    }
    const std::unique_ptr<uint64_t[]> zh(new uint64_t[plan.n_zhinv]);
    memcpy(zh.get(), plan.zhinv, plan.n_zhinv * 8);
    std::vector<ZOp> ops;
    std::vector<ZTerm> terms;
    if ((rc = zxp_records(a, plan, zh.get(), ops, terms))) {
        printf("error %d: %s\n", rc, g_msg);
        return 0;
    }
    if (ops.size() != plan.prog.n_instr || terms.size() != plan.n_dot_terms) return fail("record counts");

    // ---- the records' own invariants
    auto inside = [&](const uint64_t *q, uint32_t ncol) {  // a column (ncol of them, ld apart) of one section
        for (int k = 0; k < 12; k++)
            if (sec_words[k] && q >= S.sec[k] && q < S.sec[k] + sec_words[k]) {
                const size_t off = (size_t)(q - S.sec[k]);
                return off % S.ld[k] == 0 && off / S.ld[k] + ncol <= S.ncols[k];
            }
        return false;
    };
    auto operand_ok = [&](uint32_t kind, const uint64_t *ptr, int32_t ii, uint32_t ld, const uint64_t *imm) {
        const size_t lds_words = ((size_t)plan.prog.n_tmp1 + 3 * (size_t)plan.prog.n_tmp3) * 64;
        switch (kind) {
        case DK_T1: return ii >= 0 && ii % 64 == 0 && (size_t)ii + 64 <= lds_words;
        case DK_T3: return ii >= 0 && ii % 64 == 0 && (size_t)ii + 192 <= lds_words;
        case DK_C1: return inside(ptr, 1);
        case DK_C3: return inside(ptr, 3) && [&] {
            for (int k = 0; k < 12; k++)
                if (sec_words[k] && ptr >= S.sec[k] && ptr < S.sec[k] + sec_words[k]) return ld == S.ld[k];
            return false;
        }();
        case DK_IMM1:
        case DK_IMM3: return imm[0] < P && imm[1] < P && imm[2] < P;
        case DK_X: return true;
        case DK_I3: return ptr && (ptr == a.xdiv || ptr == a.xdivw);
        case DK_ZI: return ptr == zh.get() && (uint32_t)ii == plan.n_zhinv - 1;
        default: return false;
        }
    };
    for (const ZOp &z : ops) {
        if (z.op > ZXP_DOT3) return fail("record op");
        if (z.op >= ZXP_DOT1) {
            if (z.ia < 0 || z.ib < 0 || (size_t)z.ia + (size_t)z.ib > terms.size()) return fail("DOT term range");
            const uint32_t *k0 = reinterpret_cast<const uint32_t *>(z.ima);
            for (int j = 0; j < 3; j++)
                if (k0[3 * j] >> 22 || k0[3 * j + 1] >> 21 || limbs3(k0 + 3 * j) >= P) return fail("DOT constant");
        } else {
            if (!operand_ok(z.ka, z.pa, z.ia, z.lda, z.ima)) return fail("operand a");
            if (z.op != ZXP_COPY && !operand_ok(z.kb, z.pb, z.ib, z.ldb, z.imb)) return fail("operand b");
        }
        const uint64_t none[3] = {0, 0, 0};
        if (z.kd > DK_C3 || !operand_ok(z.kd, z.pd, z.id, z.ldd, none)) return fail("destination");
    }
    for (const ZTerm &t : terms) {
        if (t.kind != DK_T1 && t.kind != DK_C1) return fail("term kind");
        const uint64_t none[3] = {0, 0, 0};
        if (!operand_ok(t.kind, t.ptr, t.ii, 0, none)) return fail("term source");
        for (int j = 0; j < 3; j++) {
            for (int h = 0; h < 2; h++)
                if (t.c[j][3 * h] >> 22 || t.c[j][3 * h + 1] >> 21) return fail("term limb width");
            const uint64_t c = limbs3(t.c[j]);
            if (c >= P || limbs3(t.c[j] + 3) != mul(c, 1ULL << 32)) return fail("term coefficient");
        }
    }

    // ---- replay
    Replay R{a, plan, ops, terms, {}, {}, a.wrap ? ((uint64_t)dom - 1) : ~0ULL};
    R.lds.assign(std::max<size_t>(1, (size_t)plan.prog.n_tmp1 + 3 * (size_t)plan.prog.n_tmp3) * 64, 0);
    R.x.resize(dom);
    const uint64_t om = h_w(a.log_omega);
    uint64_t xi = a.x_start % P;
    for (size_t i = 0; i < dom; i++, xi = mul(xi, om)) R.x[i] = xi;
    for (size_t i = 0; i < dom; i++) R.row(i);

    FILE *f = fopen(argv[2], "wb");
    if (!f) return fail("cannot write the output");
    for (int k = 0; k < 12; k++)
        if (sec_words[k] && fwrite(S.sec[k], 8, sec_words[k], f) != sec_words[k]) return fail("short write");
    fclose(f);
    puts("replayed");
    return 0;
}
