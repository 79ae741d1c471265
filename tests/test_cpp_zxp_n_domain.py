"""zkgpu_zxp_to_n_domain (csrc/zxp_n_domain.cpp) as plain host code under the
host sanitizers: tests/cpp/zxp_n_domain_check.cpp links the source with
-fsanitize=address,undefined and runs as a child process over operand and
instruction tables of exact size.  The accepted programs give the expected
operands, every refused one the library's message.  CPU only."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zkevm-prover_amd", "csrc")
ERR = "error -2: zxp_to_n_domain: "
ZI_USE = "uses ZI other than as a factor of a product stored to SEC_Q_2NS"

EXPECTED = [
    ("base", "ok"),
    ("extend_bits_0", "ok"),
    ("extend_bits_2", "ok"),
    ("zi_first_factor", "ok"),
    ("shift_1_at_extend_bits_1", ERR + "operand 3: row shift 1 is no multiple of 2"),
    ("negative_shift_odd", ERR + "operand 4: row shift -3 is no multiple of 2"),
    ("zi_feeds_a_temporary", ERR + "instruction 7 " + ZI_USE),
    ("zi_added", ERR + "instruction 8 " + ZI_USE),
    ("zi_squared", ERR + "instruction 8 " + ZI_USE),
    ("zi_written", ERR + "instruction 7 writes ZI"),
    ("no_zi", ERR + "no product by ZI is stored to SEC_Q_2NS: not a quotient program"),
    ("read_of_q", ERR + "operand 12 reads SEC_Q_2NS"),
    ("q_shifted_store", ERR + "operand 12 stores to SEC_Q_2NS at row shift 2"),
    ("store_to_cm1", ERR + "operand 2 stores to section 5"),
    ("eval", ERR + "operand 9 of kind 8"),
    ("xdiv", ERR + "operand 9 of kind 9"),
    ("xdivw", ERR + "operand 9 of kind 10"),
    ("kind_unknown", ERR + "operand 7 of kind 13"),
    ("n_section", ERR + "operand 2 names section 0"),
    ("cm4_section", ERR + "operand 6 names section 8"),
    ("f_section", ERR + "operand 5 names section 11"),
    ("section_unknown", ERR + "operand 6 names section 12"),
    ("instr_a_range", ERR + "instruction 2 out of range"),
    ("instr_b_range", ERR + "instruction 0 out of range"),
    ("instr_dst_range", ERR + "instruction 8 out of range"),
    ("instr_op", ERR + "instruction 3 out of range"),
    ("empty", ERR + "no product by ZI is stored to SEC_Q_2NS: not a quotient program"),
]


@pytest.fixture(scope="module")
def check_bin(tmp_path_factory):
    d = tmp_path_factory.mktemp("zxp_n_domain_check")
    out = str(d / "zxp_n_domain_check")
    subprocess.check_call(
        # (the sanitizer runtimes linked statically: the program needs no place in a preload list)
        ["g++", "-O1", "-g", "-std=c++20", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         "-static-libasan", "-static-libubsan", "-o", out, os.path.join(ROOT, "tests/cpp/zxp_n_domain_check.cpp"),
         os.path.join(CSRC, "zxp_n_domain.cpp")])
    return out


def test_accepted_and_refused_under_the_host_sanitizers(check_bin):
    r = subprocess.run([check_bin], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.splitlines() == ["%s: %s" % e for e in EXPECTED]
