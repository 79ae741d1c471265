"""zkgpu_zxp_split_constraints (csrc/zxp_split.cpp) as plain host code under
the host sanitizers: tests/cpp/zxp_split_check.cpp links the source with
-fsanitize=address,undefined and runs as a child process over input and output
tables of exactly the documented sizes.  The accepted programs give the
expected tapped program and term table, every refused one the library's
message.  CPU only."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zkevm-prover_amd", "csrc")
ERR = "error -2: zxp_split: "
OTHER = "multiplies a combination by something other than the combination challenge"
NOT_Q = "stores a combination to a column other than q (SEC_Q_2NS, column 0, shift 0)"

EXPECTED = [
    ("base", "ok"),
    ("literal_one_for_zi", "ok"),
    ("copy_to_q", "ok"),
    ("product_that_feeds_nothing", "ok"),
    ("spoiled_value_added", ERR + "instruction 4 " + OTHER),
    ("two_taps_per_instruction", "ok"),
    ("product_by_another_challenge", ERR + "instruction 4 " + OTHER),
    ("product_of_two_combinations", ERR + "instruction 5 " + OTHER),
    ("zi_into_a_temporary", ERR + "no combination is stored to SEC_Q_2NS"),
    ("tmp1_destination", ERR + "instruction 3 writes a combination to a TMP1 slot"),
    ("q_column_3", ERR + "instruction 6 " + NOT_Q),
    ("cm1_column", ERR + "instruction 6 " + NOT_Q),
    ("read_only_destination", ERR + "instruction 6 writes a combination to an operand of kind 4"),
    ("q_by_a_sum", ERR + "instruction 6 stores a combination to q other than by a COPY or a product by ZI or 1"),
    ("alpha_free_store_to_q", ERR + "instruction 6 stores a value free of the combination challenge to SEC_Q_2NS"),
    ("second_store_to_q", ERR + "instruction 7 is a second store to q"),
    ("shared_term", ERR + "instruction 5 combines two combinations that share term 0"),
    ("source_out_of_range", ERR + "instruction 2 out of range"),
    ("second_source_out_of_range", ERR + "instruction 0 out of range"),
    ("destination_out_of_range", ERR + "instruction 6 out of range"),
    ("unknown_op", ERR + "instruction 3 out of range"),
    ("no_store", ERR + "no combination is stored to SEC_Q_2NS"),
    ("challenge_out_of_range", ERR + "challenge 8 out of range"),
    ("empty", ERR + "no combination is stored to SEC_Q_2NS"),
]


@pytest.fixture(scope="module")
def check_bin(tmp_path_factory):
    d = tmp_path_factory.mktemp("zxp_split_check")
    out = str(d / "zxp_split_check")
    subprocess.check_call(
        # (the sanitizer runtimes linked statically: the program needs no place in a preload list)
        ["g++", "-O1", "-g", "-std=c++20", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         "-static-libasan", "-static-libubsan", "-o", out, os.path.join(ROOT, "tests/cpp/zxp_split_check.cpp"),
         os.path.join(CSRC, "zxp_split.cpp")])
    return out


def test_accepted_and_refused_under_the_host_sanitizers(check_bin):
    r = subprocess.run([check_bin], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.splitlines() == ["%s: %s" % e for e in EXPECTED]
