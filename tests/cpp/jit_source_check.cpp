// Stand-alone run of the expression-kernel source generator: the host-only
// sources of the library (zxp_compile, zxp_segment, zxp_jit_source, gl_host)
// linked into a plain program, so the generator runs under the host
// sanitizers with nothing loaded into Python (tests/test_cpp_jit_source.py).
//
// usage: jit_source_check PROGRAM.bin
// PROGRAM.bin (u64 words): magic, n_instr, n_opnd, n_tmp1, n_tmp3, n_publics,
// n_evals, then instr and opnd (u32 x 4 each, padded to a whole word), 24
// challenge words, the publics, 3 n_evals eval words.
// Prints what zkgpu_zxp_jit_source returns for the same program with an empty
// code-object cache: the source (segments with their separator lines), or
// "unsupported program shape".
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../zkevm-prover_amd/csrc/zxp_jit_source.hpp"
#include "../../zkevm-prover_amd/csrc/zxp_segment.hpp"

namespace zk {
int set_error(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
    fputc('\n', stderr);
    return code;
}
}  // namespace zk

using namespace zk;

static int fail(const char *what)
{
    fprintf(stderr, "jit_source_check: %s\n", what);
    return 2;
}

int main(int argc, char **argv)
{
    if (argc != 2) return fail("usage: jit_source_check PROGRAM.bin");
    std::vector<uint64_t> w;
    {
        FILE *f = fopen(argv[1], "rb");
        if (!f) return fail("cannot open the program");
        uint64_t buf[4096];
        for (size_t n; (n = fread(buf, 8, 4096, f)) > 0;) w.insert(w.end(), buf, buf + n);
        fclose(f);
    }
    if (w.size() < 7 || w[0] != 0x4a4954535243ULL) return fail("bad header");
    const uint32_t n_instr = (uint32_t)w[1], n_opnd = (uint32_t)w[2], n_tmp1 = (uint32_t)w[3], n_tmp3 = (uint32_t)w[4],
                   n_pub = (uint32_t)w[5], n_ev = (uint32_t)w[6];
    const size_t o_instr = 7, o_opnd = o_instr + 2 * (size_t)n_instr, o_ch = o_opnd + 2 * (size_t)n_opnd,
                 o_pub = o_ch + 24, o_ev = o_pub + n_pub;
    if (w.size() != o_ev + 3 * (size_t)n_ev) return fail("bad length");
    // exact-size copies, so a read past a table's end is seen
    const std::vector<uint64_t> instr(w.begin() + o_instr, w.begin() + o_opnd), opnd(w.begin() + o_opnd, w.begin() + o_ch),
        chal(w.begin() + o_ch, w.begin() + o_pub), pub(w.begin() + o_pub, w.begin() + o_ev), ev(w.begin() + o_ev, w.end());
    zxp_compiled cp;
    if (zkgpu_zxp_compile(instr.data(), n_instr, opnd.data(), n_opnd, n_tmp1, n_tmp3, chal.data(), pub.data(), n_pub,
                          ev.data(), n_ev, 0, &cp))
        return fail("zkgpu_zxp_compile");
    // placeholder sections and scratch: pointers are kernel inputs, not part of the source
    static uint64_t dummy;
    zkgpu_sections S;
    for (int k = 0; k < 12; k++) {
        S.sec[k] = &dummy;
        S.ld[k] = 1;
        S.ncols[k] = 0;
    }
    const ZxpJitIn J = zxp_jit_in(cp, &S, chal.data(), pub.data(), ev.data());
    std::vector<ZxpSegment> seg;
    const uint32_t nseg = segments_for(cp);
    uint32_t n_scratch = 0;
    if (nseg > 1 && zxp_segment(cp, nseg, seg, n_scratch)) return fail("zxp_segment");
    std::string text;
    ZxpJitSource out;
    for (size_t j = 0; j < (nseg > 1 ? seg.size() : 1); j++) {
        ZxpJitIn K = J;
        if (nseg > 1) {  // a segment as the library first builds it: code blocks, 4 waves per SIMD
            K.ins = seg[j].instr.data();
            K.n_instr = (uint32_t)seg[j].instr.size();
            K.opnd = seg[j].opnd.data();
            K.n_opnd = (uint32_t)seg[j].opnd.size();
            K.terms = seg[j].term.data();
            K.force_split = 1;
            K.waves_per_eu = 4;
            K.scratch = &dummy;
            K.scratch_ld = 1;
            if (seg.size() > 1) text += "// ---- segment " + std::to_string(j) + " of " + std::to_string(seg.size()) + "\n";
        }
        if (zxp_jit_build_source(K, out)) {
            puts("unsupported program shape");
            return 0;
        }
        text += out.src;
    }
    fwrite(text.data(), 1, text.size(), stdout);
    return 0;
}
