"""The host side of an expression evaluation (csrc/zxp_prepare.cpp: argument
checks, plan, interpreter records) as plain host code under the host
sanitizers: tests/cpp/zxp_prepare_check.cpp links the library's host-only
sources with -fsanitize=address,undefined and runs as a child process on the
cases dumped here.  Every argument check rejects its own defect with the
library's message, and the records of real programs, replayed on the host over
sections of exact size, give what the oracle computes from the SOURCE program,
bit for bit.  CPU only."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zkevm-prover_amd", "csrc")
sys.path[:0] = [os.path.dirname(os.path.abspath(__file__))]
MAGIC = 0x5a5850505245
P = 0xFFFFFFFF00000001
ERR_ARG = -2  # ZKGPU_ERR_ARG (include/zkgpu.h)
TMP1, TMP3, COL, COL3, LIT, CHAL, PUB, X, EVAL, XDIV, XDIVW, ZI = range(12)
ADD, SUB, MUL, COPY = range(4)
# (ZKGPU_ZXP_FUSE, ZKGPU_ZXP_MAX_TERMS, ZKGPU_ZXP_JIT): the interpreter on the compiled program at the default and
# at a tiny term cap, and on the unfused source program
INTERPRETER = [("1", "0", "0"), ("1", "3", "0"), ("0", "0", "0")]


@pytest.fixture(scope="module")
def check_bin(tmp_path_factory):
    d = tmp_path_factory.mktemp("zxp_prepare_check")
    with open(os.path.join(CSRC, "gl_device.hpp")) as f:  # as the Makefile's build/gl_device_src.inc
        (d / "gl_device_src.inc").write_text('R"ZKSRC(\n' + f.read() + ')ZKSRC"\n')
    out = str(d / "zxp_prepare_check")
    subprocess.check_call(
        # (the sanitizer runtimes linked statically: the program needs no place in a preload list)
        ["g++", "-O1", "-g", "-std=c++20", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         "-static-libasan", "-static-libubsan",
         "-I" + str(d), "-o", out, os.path.join(ROOT, "tests/cpp/zxp_prepare_check.cpp")]
        + [os.path.join(CSRC, f) for f in ("zxp_prepare.cpp", "zxp_compile.cpp", "zxp_jit_source.cpp", "gl_host.cpp")]
        + ["-lpthread"])
    return out


class Case:
    """One call of zkgpu_zxp_eval_dev / _block_dev.  sections: {index: (ld, ncols)}
    with random data, or {index: (ld, ncols, address)} for a placeholder."""

    def __init__(self, ins, opn, n_tmp1, n_tmp3, sections, log_dom, log_omega=None, wrap=1, extend_bits=0,
                 x_start=1, n_publics=1, n_evals=1, xdiv=1, xdivw=1, seed=1):
        self.ins = np.array(ins, np.uint32).reshape(-1, 4)
        self.opn = np.array(opn, np.int64).astype(np.uint32).reshape(-1, 4)
        self.n_tmp1, self.n_tmp3 = n_tmp1, n_tmp3
        self.sections = dict(sections)
        self.log_dom, self.log_omega = log_dom, log_dom if log_omega is None else log_omega
        self.wrap, self.extend_bits, self.x_start = wrap, extend_bits, x_start
        self.xdiv, self.xdivw = xdiv, xdivw
        rng = np.random.default_rng(seed)
        self.chal = rand_gl(rng, (8, 3))
        self.pub = rand_gl(rng, n_publics)
        self.evals = rand_gl(rng, (n_evals, 3))
        self.data = None

    def fill(self, seed=2):
        """row-major section data (the oracle's layout) and the xdiv tables"""
        rng = np.random.default_rng(seed)
        self.data = {k: rand_gl(rng, (s[0], s[1])) for k, s in sorted(self.sections.items()) if len(s) == 2}
        self.xd = rand_gl(rng, (1 << self.log_dom, 3))
        self.xdw = rand_gl(rng, (1 << self.log_dom, 3))
        return self

    def dump(self, path):
        if self.data is None:
            self.fill()
        hdr = [MAGIC, self.ins.shape[0], self.opn.shape[0], self.n_tmp1, self.n_tmp3, self.pub.size,
               self.evals.shape[0], self.log_dom, self.log_omega, self.wrap, self.extend_bits, self.x_start,
               self.xdiv, self.xdivw]
        for k in range(12):
            s = self.sections.get(k)
            hdr += [0, 0, 0] if s is None else [1 if len(s) == 2 else s[2], s[0], s[1]]
        parts = [np.array(hdr, np.uint64), self.ins, self.opn, self.chal, self.pub, self.evals]
        parts += [np.ascontiguousarray(a.T) for a in self.data.values()]  # column-major
        parts += [t for t, how in ((self.xd, self.xdiv), (self.xdw, self.xdivw)) if how == 1]
        with open(path, "wb") as f:
            for a in parts:
                f.write(np.ascontiguousarray(a).tobytes())

    def outputs(self, path):
        """the sections the check program wrote, row-major"""
        flat = np.fromfile(path, np.uint64)
        out, at = {}, 0
        for k, a in self.data.items():
            if a.size:
                out[k] = flat[at:at + a.size].reshape(a.shape[1], a.shape[0]).T
                at += a.size
        assert at == flat.size
        return out

    def oracle_sections(self, oracle, zh_n=None):
        """oc_zxp_eval of the source program on copies of the data"""
        S = {k: a.copy() for k, a in self.data.items()}
        dom = 1 << self.log_dom
        eb = self.extend_bits
        x = np.zeros(dom, np.uint64)
        p = oracle._p
        oracle.lib().oc_powers(p(x), self.x_start, oracle.gl_w(self.log_omega), dom)
        n = (1 << (self.log_omega - eb)) if zh_n is None else zh_n
        wE = oracle.gl_w(eb)
        zh = np.array([pow((pow(7, n, P) * pow(wE, i, P) - 1) % P, P - 2, P) for i in range(1 << eb)], np.uint64)
        sp = (ctypes.c_void_p * 12)()
        strides = np.zeros(12, np.uint64)
        for k, a in S.items():
            sp[k] = a.ctypes.data
            strides[k] = a.shape[1]
        ins, opn = np.ascontiguousarray(self.ins), np.ascontiguousarray(self.opn)
        oracle.lib().oc_zxp_eval(ctypes.c_void_p(ins.ctypes.data), ins.shape[0], ctypes.c_void_p(opn.ctypes.data),
                                 self.n_tmp1, self.n_tmp3, ctypes.cast(sp, ctypes.c_void_p),
                                 ctypes.c_void_p(strides.ctypes.data), dom, p(self.chal), p(self.pub), p(self.evals),
                                 p(x), p(self.xd), p(self.xdw), p(zh), zh.size)
        return S


def rand_gl(rng, shape):
    return rng.integers(0, 2**63, size=shape, dtype=np.uint64)


def run(check_bin, case, tmp_path, mode=None):
    """-> (the check program's stdout lines, path of its output)"""
    case.dump(tmp_path / "case.bin")
    env = {k: v for k, v in os.environ.items() if not k.startswith("ZKGPU_ZXP_")}
    if mode:
        env.update(ZKGPU_ZXP_FUSE=mode[0], ZKGPU_ZXP_MAX_TERMS=mode[1], ZKGPU_ZXP_JIT=mode[2])
    r = subprocess.run([check_bin, str(tmp_path / "case.bin"), str(tmp_path / "out.bin")], capture_output=True,
                       text=True, timeout=120, env=env)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-4000:]
    return r.stdout.splitlines(), tmp_path / "out.bin"


def check_vs_oracle(check_bin, oracle, case, tmp_path, mode, first_line="replayed", zh_n=None):
    if case.data is None:
        case.fill()
    want = case.oracle_sections(oracle, zh_n)
    lines, out = run(check_bin, case, tmp_path, mode)
    assert lines == ([first_line, "replayed"] if first_line != "replayed" else ["replayed"]), lines
    got = case.outputs(out)
    assert sorted(got) == sorted(k for k, a in want.items() if a.size)
    for k, a in got.items():
        assert np.array_equal(a, want[k]), "section %d" % k


# ---- every argument check: a small valid program that reads each operand kind, one defect at a time
def base_case(**kw):
    opn = [(TMP1, 0, 0, 0), (TMP3, 0, 0, 0), (COL, 0, 0, 1), (COL3, 1, 0, 0), (LIT, 5, 0, 0), (CHAL, 1, 0, 0),
           (PUB, 0, 0, 0), (X, 0, 0, 0), (EVAL, 0, 0, 0), (XDIV, 0, 0, 0), (XDIVW, 0, 0, 0), (ZI, 0, 0, 0),
           (COL, 2, 0, 0), (COL3, 2, 1, 0)]
    ins = [(MUL, 0, 2, 4), (ADD, 0, 0, 6), (MUL, 0, 0, 7), (MUL, 0, 0, 11), (COPY, 12, 0, 0), (MUL, 1, 3, 5),
           (ADD, 1, 1, 8), (MUL, 1, 1, 9), (SUB, 1, 1, 10), (ADD, 13, 1, 0)]
    args = dict(n_tmp1=1, n_tmp3=1, sections={0: (17, 1), 1: (17, 3), 2: (17, 4)}, log_dom=4, extend_bits=1, x_start=7)
    args.update(kw)
    return Case(ins, opn, **args)


def _set(field, row, col, value):
    def mutate(c):
        getattr(c, field)[row, col] = np.int64(value).astype(np.uint32)
    return mutate


def _section(k, *spec):
    def mutate(c):
        if spec:
            c.sections[k] = spec
        else:
            del c.sections[k]
    return mutate


def _attr(**kw):
    def mutate(c):
        for k, v in kw.items():
            setattr(c, k, v)
    return mutate


# (what to change, keyword arguments of the case, the library's message: csrc/zxp_prepare.cpp)
REJECTED = {
    "instr_a_range": (_set("ins", 2, 2, 14), {}, "zxp: instruction 2 out of range"),
    "instr_b_range": (_set("ins", 0, 3, 14), {}, "zxp: instruction 0 out of range"),
    "instr_dst_range": (_set("ins", 9, 1, 14), {}, "zxp: instruction 9 out of range"),
    "instr_op": (_set("ins", 3, 0, 4), {}, "zxp: instruction 3 out of range"),
    "tmp1_slot": (_set("opn", 0, 1, 1), {}, "zxp: operand 0 (kind 0) invalid"),
    "tmp3_slot": (_set("opn", 1, 1, 1), {}, "zxp: operand 1 (kind 1) invalid"),
    "col_past_ncols": (_set("opn", 2, 2, 1), {}, "zxp: operand 2 (kind 2) invalid"),
    "col3_past_ncols": (_set("opn", 3, 2, 1), {}, "zxp: operand 3 (kind 3) invalid"),
    "section_index": (_set("opn", 2, 1, 12), {}, "zxp: operand 2 (kind 2) invalid"),
    "section_null": (_section(0), {}, "zxp: operand 2 (kind 2) invalid"),
    "ld_short_of_domain": (_section(1, 15, 3), {}, "zxp: operand 3 (kind 3) invalid"),
    "ld_short_of_halo": (_section(0, 16, 1), {"wrap": 0}, "zxp: operand 2 (kind 2) invalid"),
    "negative_shift_in_block": (_set("opn", 2, 3, -1), {"wrap": 0}, "zxp: operand 2 (kind 2) invalid"),
    "challenge_index": (_set("opn", 5, 1, 8), {}, "zxp: operand 5 (kind 5) invalid"),
    "public_index": (_set("opn", 6, 1, 1), {}, "zxp: operand 6 (kind 6) invalid"),
    "eval_index": (_set("opn", 8, 1, 1), {}, "zxp: operand 8 (kind 8) invalid"),
    "xdiv_null": (_attr(xdiv=0), {}, "zxp: operand 9 (kind 9) invalid"),
    "xdivw_null": (_attr(xdivw=0), {}, "zxp: operand 10 (kind 10) invalid"),
    "kind_unknown": (_set("opn", 4, 0, 13), {}, "zxp: operand 4 (kind 13) invalid"),
    "kind_compiled_only": (_set("opn", 4, 0, 12), {}, "zxp: operand 4 (kind 12) invalid"),
    "log_dom_over_log_omega": (_attr(), {"log_dom": 5, "log_omega": 4, "sections": {0: (33, 1), 1: (33, 3), 2: (33, 4)}},
                               "zxp: domain too large"),
    "log_omega_over_28": (_attr(), {"log_omega": 29}, "zxp: domain too large"),
    "extend_bits_over_log_omega": (_attr(), {"extend_bits": 5}, "zxp: extend bits exceed the domain"),
    "extend_bits_over_6": (_attr(), {"log_omega": 8, "extend_bits": 7}, "zxp: extend bits > 6"),
    # (placeholder address: nothing is dereferenced before the check)
    "stride_over_2_32": (_section(0, 1 << 32, 1, 0x10000), {}, "zxp: section 0 stride exceeds 2^32"),
    "destination_literal": (_set("ins", 4, 1, 4), {}, "zxp: instruction 4 writes a read-only operand"),
}


@pytest.mark.parametrize("mode", INTERPRETER, ids="-".join)
def test_base_case_is_valid(check_bin, oracle, tmp_path, mode):
    """the program the rejections start from, as a whole domain and as a row
    block with one halo row and a negative shift that wraps"""
    check_vs_oracle(check_bin, oracle, base_case(), tmp_path, mode)
    c = base_case()
    c.opn[2, 3] = np.int64(-1).astype(np.uint32)
    check_vs_oracle(check_bin, oracle, c, tmp_path, mode)
    lines, _ = run(check_bin, base_case(wrap=0), tmp_path, mode)  # (a block's halo is the caller's: not the oracle's rows)
    assert lines == ["replayed"]


@pytest.mark.parametrize("name", sorted(REJECTED))
def test_rejected(check_bin, tmp_path, name):
    mutate, kw, message = REJECTED[name]
    c = base_case(**kw)
    mutate(c)
    # the checks of the arguments do not depend on the path; a destination's kind is checked on the program
    # that runs, by the compiler or after the slot packing
    for mode in ([None] + INTERPRETER if name == "destination_literal" else [None]):
        lines, _ = run(check_bin, c, tmp_path, mode)
        assert lines == ["error %d: %s" % (ERR_ARG, message)]


def test_lds_bound_fusion_off(check_bin, oracle, tmp_path):
    """The interpreter's temporaries live in 160 KiB of LDS: 320 slots of 64
    rows.  n live base temporaries and the one extension slot every program
    has take n + 3."""
    def live(n):
        opn = [(COL, 0, 0, 0), (LIT, 3, 0, 0), (COL, 1, 0, 0)] + [(TMP1, k, 0, 0) for k in range(n)]
        ins = [(MUL, 3 + k, 0, 1) for k in range(n)] + [(ADD, 3, 3, 3 + k) for k in range(1, n)] + [(COPY, 2, 3, 0)]
        return Case(ins, opn, n, 1, {0: (16, 1), 1: (16, 1)}, log_dom=4)
    check_vs_oracle(check_bin, oracle, live(317), tmp_path, ("0", "0", "0"))
    lines, _ = run(check_bin, live(318), tmp_path, ("0", "0", "0"))
    assert lines == ["error %d: zxp: 321 temp slots exceed LDS" % ERR_ARG]


# ---- the records of real programs
@pytest.fixture(scope="module")
def stark():
    from zkgpu.synthetic import SyntheticStark
    return SyntheticStark(n_bits=9, blowup_bits=1, t=8, m=3, n_free=4, n_lookups=2, n_queries=8)


@pytest.mark.parametrize("name", ["step1", "step2", "step3prev", "step42ns", "step52ns"])
@pytest.mark.parametrize("mode", INTERPRETER, ids="-".join)
def test_records_vs_oracle(check_bin, oracle, stark, tmp_path, name, mode):
    """the programs and inputs of tests/test_gpu_stark.py::test_zxp_programs_vs_oracle"""
    inst, prog = stark, stark.programs[name]
    logd = inst.n_bits_ext if prog.domain_ext else inst.n_bits
    dom = 1 << logd
    widths = {0: inst.n_cm1, 1: inst.n_cm2, 2: inst.n_cm3, 3: inst.n_tmp, 4: inst.n_const, 5: inst.n_cm1,
              6: inst.n_cm2, 7: inst.n_cm3, 8: inst.n_cm4, 9: inst.n_const, 10: 3, 11: 3}
    ins, opn = prog.arrays()
    c = Case(ins, opn, max(prog.n_tmp1, 1), max(prog.n_tmp3, 1), {k: (dom, w) for k, w in widths.items()}, logd,
             extend_bits=inst.blowup_bits, x_start=7 if prog.domain_ext else 1, n_publics=inst.n_publics,
             n_evals=len(inst.evmap), xdiv=int(prog.domain_ext), xdivw=int(prog.domain_ext),
             seed=sum(map(ord, name)))
    check_vs_oracle(check_bin, oracle, c, tmp_path, mode, zh_n=dom >> inst.blowup_bits if prog.domain_ext else dom)


@pytest.mark.parametrize("name", ["cross_row_read_after_write", "mixed_stored_triple"])
def test_records_of_the_shapes_left_to_the_interpreter(check_bin, oracle, tmp_path, name):
    """ZKGPU_ZXP_JIT=2 plans the compiled kernels, the source generator declines
    the shape, and the interpreter's records come from that same plan."""
    import jit_shape_cases as js
    prog = js.UNSUPPORTED[name]()
    ins, opn = prog.arrays()
    c = Case(ins, opn, max(prog.n_tmp1, 1), max(prog.n_tmp3, 1), {k: (128, w) for k, w in js.WIDTHS.items()}, 7)
    c.fill()
    if name == "cross_row_read_after_write":
        # row i reads cm2[0] of row i + 1, which that row stores, and the oracle's rows run in parallel: the
        # column already holds the product, so the read has one value (as tests/test_gpu_dot_cases.py does)
        a = c.data[js.SEC_CM1_N]
        c.data[js.SEC_CM2_N][:, 0] = [int(x) * int(y) % P for x, y in zip(a[:, 0], a[:, 1])]
    check_vs_oracle(check_bin, oracle, c, tmp_path, ("1", "0", "2"), first_line="jit: unsupported program shape")
