"""The host side of zkgpu_zxp_eval_rows_dev (csrc/zxp_prepare.cpp with
ZxpArgs::row_list: the row-list argument checks of zxp_validate, the plan, the
interpreter's records) as plain host code under the host sanitizers:
tests/cpp/zxp_rows_check.cpp links the library's host-only sources with
-fsanitize=address,undefined and runs as a child process over tables of exact
size.  The accepted calls are planned for the interpreter and store inside
their compact section; every refused one gives the library's message.  CPU
only."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zkevm-prover_amd", "csrc")
ERR = "error -2: "

EXPECTED = [
    ("base", "ok"),
    ("never_the_compiled_kernels", "ok"),
    ("fusion_off", "ok"),
    ("n_rows_4096", "ok"),
    ("n_rows_4097", ERR + "zxp rows: 4097 rows exceed 4096"),
    ("one_row", "ok"),
    ("null_rows", ERR + "zxp rows: null row list"),
    ("null_rows_and_no_rows", ERR + "zxp rows: null row list"),
    ("store_section_shorter_than_the_list", ERR + "zxp rows: section 10 is stored to and holds 4 rows, not 5"),
    ("read_section_shorter_than_the_domain", ERR + "zxp: operand 2 (kind 2) invalid"),
    ("store_past_the_columns", ERR + "zxp: operand 7 (kind 3) invalid"),
    ("store_at_a_row_shift", ERR + "zxp rows: instruction 3 stores at row shift 1"),
    ("store_at_a_negative_row_shift", ERR + "zxp rows: instruction 5 stores at row shift -1"),
    ("read_of_the_stored_section", ERR + "zxp rows: section 10 is both read and stored to"),
    ("store_section_index", ERR + "zxp: operand 6 (kind 2) invalid"),
    ("read_section_index", ERR + "zxp: operand 2 (kind 2) invalid"),
    ("instr_dst_range", ERR + "zxp: instruction 3 out of range"),
    ("instr_a_range", ERR + "zxp: instruction 0 out of range"),
    ("instr_b_range", ERR + "zxp: instruction 0 out of range"),
    ("store_to_a_read_section", ERR + "zxp rows: section 0 is both read and stored to"),
    ("unused_operand_of_the_stored_section", "ok"),
]


@pytest.fixture(scope="module")
def check_bin(tmp_path_factory):
    d = tmp_path_factory.mktemp("zxp_rows_check")
    with open(os.path.join(CSRC, "gl_device.hpp")) as f:  # as the Makefile's build/gl_device_src.inc
        (d / "gl_device_src.inc").write_text('R"ZKSRC(\n' + f.read() + ')ZKSRC"\n')
    out = str(d / "zxp_rows_check")
    subprocess.check_call(
        # (the sanitizer runtimes linked statically: the program needs no place in a preload list)
        ["g++", "-O1", "-g", "-std=c++20", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         "-static-libasan", "-static-libubsan", "-I" + str(d), "-o", out,
         os.path.join(ROOT, "tests/cpp/zxp_rows_check.cpp")]
        + [os.path.join(CSRC, f) for f in ("zxp_prepare.cpp", "zxp_compile.cpp", "zxp_jit_source.cpp", "gl_host.cpp")]
        + ["-lpthread"])
    return out


def test_accepted_and_refused_under_the_host_sanitizers(check_bin):
    env = {k: v for k, v in os.environ.items() if not k.startswith("ZKGPU_ZXP_")}
    r = subprocess.run([check_bin], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and r.stderr == "", (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.splitlines() == ["%s: %s" % e for e in EXPECTED]
