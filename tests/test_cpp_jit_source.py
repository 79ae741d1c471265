"""The expression-kernel source generator as plain host code under the host
sanitizers: tests/cpp/jit_source_check.cpp links the library's host-only
sources (zxp_compile, zxp_segment, zxp_jit_source, gl_host) with
-fsanitize=address,undefined and runs as a child process on a program dumped
here; its output equals zkgpu.zxp_jit_source of the same program (the library
build of the same sources)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zkevm-prover_amd", "csrc")
sys.path[:0] = [os.path.join(ROOT, "tools"), os.path.dirname(os.path.abspath(__file__))]
MAGIC = 0x4a4954535243


# The library's text for the same program, from a child process of its own:
# ZKGPU_JIT_CACHE=0 is read once per process, and with the cache on the
# library looks the occupancy re-compiles up and may print another variant.
_LIBRARY_SOURCE = """
import sys
sys.path[:0] = %r
import jit_prebuild as jp
import test_cpp_jit_source as t
import zkgpu
try:
    out = zkgpu.zxp_jit_source(t._program(sys.argv[1]), *jp.consts())
except RuntimeError as e:
    out = "unsupported program shape\\n" if "unsupported program shape" in str(e) else "error: %%s" %% e
open(sys.argv[2], "w").write(out)
"""


def _library_source(spec, path):
    here = os.path.dirname(os.path.abspath(__file__))
    code = _LIBRARY_SOURCE % ([ROOT, os.path.join(ROOT, "zkevm-prover_amd"), os.path.join(ROOT, "tools"), here],)
    env = dict(os.environ, ZKGPU_JIT_CACHE="0")
    env.pop("ZKGPU_ZXP_SEG_AB", None)
    subprocess.run([sys.executable, "-c", code, spec, str(path)], check=True, timeout=300, env=env)
    with open(path) as f:
        return f.read()


@pytest.fixture(scope="module")
def check_bin(tmp_path_factory):
    d = tmp_path_factory.mktemp("jit_source_check")
    with open(os.path.join(CSRC, "gl_device.hpp")) as f:  # as the Makefile's build/gl_device_src.inc
        (d / "gl_device_src.inc").write_text('R"ZKSRC(\n' + f.read() + ')ZKSRC"\n')
    out = str(d / "jit_source_check")
    subprocess.check_call(
        # (the sanitizer runtimes linked statically: the program needs no place in a preload list)
        ["g++", "-O1", "-g", "-std=c++20", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         "-static-libasan", "-static-libubsan",
         "-I" + str(d), "-o", out, os.path.join(ROOT, "tests/cpp/jit_source_check.cpp")]
        + [os.path.join(CSRC, f) for f in ("zxp_compile.cpp", "zxp_segment.cpp", "zxp_jit_source.cpp", "gl_host.cpp")]
        + ["-lpthread"])
    return out


def _dump(path, prog, ch, pub, ev):
    ins, opn = prog.arrays()
    chal = np.zeros(24, np.uint64)
    chal[:np.asarray(ch).size] = np.asarray(ch, np.uint64).reshape(-1)
    pub = np.asarray(pub, np.uint64).reshape(-1)
    ev = np.asarray(ev, np.uint64).reshape(-1)
    hdr = np.array([MAGIC, ins.shape[0], opn.shape[0], max(prog.n_tmp1, 1), max(prog.n_tmp3, 1), pub.size, ev.size // 3],
                   np.uint64)
    with open(path, "wb") as f:
        for a in (hdr, np.ascontiguousarray(ins, np.uint32), np.ascontiguousarray(opn, np.uint32), chal, pub, ev):
            f.write(a.tobytes())


def _program(spec):
    import jit_prebuild as jp
    import jit_shape_cases as js
    if spec in js.UNSUPPORTED:
        return js.UNSUPPORTED[spec]()
    return jp.get_program(spec)


# one split kernel; 4 segments (column cache and prefetch); fused chains;
# looped DOTs with the limbs in LDS; the two shapes left to the interpreter
@pytest.mark.parametrize("spec,segments", [
    ("shaped:step42ns:0.25", 0), ("shaped:step3:1", 4), ("shaped:step52ns:1", 0), ("stark:config4:step42ns", 0),
    ("cross_row_read_after_write", None), ("mixed_stored_triple", None)])
def test_generator_under_sanitizers(check_bin, tmp_path, spec, segments):
    import jit_prebuild as jp
    prog = _program(spec)
    ch, pub, ev = jp.consts()
    _dump(tmp_path / "prog.bin", prog, ch, pub, ev)
    env = {k: v for k, v in os.environ.items() if k != "ZKGPU_ZXP_SEG_AB"}  # (the A/B switch changes the segments)
    r = subprocess.run([check_bin, str(tmp_path / "prog.bin")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stderr == ""
    src = _library_source(spec, tmp_path / "library.txt")
    assert r.stdout == src
    if segments is None:
        assert src == "unsupported program shape\n"
        return
    assert src.count("// ---- segment ") == segments
    if spec == "shaped:step42ns:0.25":
        assert "#define ZKJIT_SPLIT 1" in src and "LC(" in src
    elif spec == "shaped:step3:1":
        assert "CS(" in src and "zpf0_0 = C(" in src
    elif spec == "shaped:step52ns:1":
        assert src.count("for (int q_") >= 3
    else:
        assert "dot_cols<3>(" in src and "#define ZKJIT_KL_LDS 1" in src
