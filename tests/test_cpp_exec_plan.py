"""The .exec planner (csrc/exec_plan.cpp) as plain host code under the host
sanitizers: tests/cpp/exec_plan_check.cpp links the source with
-fsanitize=address,undefined and runs as a child process over images of
exactly their stated length.  For an accepted image the program itself checks
every add's level against a relaxation to a fixed point, that every add reads
only slots an earlier level wrote, and how the levels are cut into launches;
a refused one gives the library's message.  CPU only."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zkevm-prover_amd", "csrc")
ERR = "error -2: exec_plan: "
LONG = "the image has %d words, not 2 + 4 x 2000 adds + 1000 x %d cells"

# accepted: depth, kernel launches of a commit (the segments + the gather), the segments
# (G: one level over the grid, t: a run of narrow levels in one workgroup)
EXPECTED = [
    ("a_random_dag", "ok levels 12 launches 2 t"),
    ("b_chain_5000", "ok levels 5000 launches 2 t"),
    ("c_grid_tail_grid", "ok levels 302 launches 4 GtG"),
    ("d_levels_T-1_T_T+1", "ok levels 3 launches 3 tG"),
    ("d_at_tail_256", "ok levels 3 launches 4 GGG"),
    ("d_at_tail_1023", "ok levels 3 launches 4 tGG"),
    ("e_no_adds", "ok levels 0 launches 1 "),
    ("e_nothing_at_all", "ok levels 0 launches 1 "),
    ("slots_2^32-1", "ok levels 1 launches 2 t"),
    ("one_word_short", ERR + LONG % (20001, 12)),
    ("one_word_long", ERR + LONG % (20003, 12)),
    ("another_n_cols", ERR + LONG % (20002, 13)),
    ("no_header", ERR + "the image has 1 words, less than its 2-word header"),
    ("header_that_wraps", ERR + "the image has 2 words, not 2 + 4 x 4611686018427387904 adds + 0 x 12 cells"),
    ("forward_reference", ERR + "add 5 reads slot 307, not below its own slot 305"),
    ("self_reference", ERR + "add 5 reads slot 305, not below its own slot 305"),
    ("smap_past_the_slots", ERR + "sMap cell (row 7, column 3) reads slot 2300 of 2300"),
    ("slots_2^32", ERR + "size_witness + nAdds = 4294967295 + 1 does not fit 32-bit slot indices"),
    ("witness_2^32", ERR + "size_witness + nAdds = 4294967296 + 0 does not fit 32-bit slot indices"),
    ("no_columns", ERR + "n_cols is 0"),
    ("no_witness", ERR + "size_witness is 0"),
    ("tail_too_wide", ERR + "tail width 1025 above 1024"),
]


@pytest.fixture(scope="module")
def check_bin(tmp_path_factory):
    d = tmp_path_factory.mktemp("exec_plan_check")
    out = str(d / "exec_plan_check")
    subprocess.check_call(
        # (the sanitizer runtimes linked statically: the program needs no place in a preload list)
        ["g++", "-O1", "-g", "-std=c++20", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         "-static-libasan", "-static-libubsan", "-o", out, os.path.join(ROOT, "tests/cpp/exec_plan_check.cpp"),
         os.path.join(CSRC, "exec_plan.cpp")])
    return out


def test_plans_and_refusals_under_the_host_sanitizers(check_bin):
    r = subprocess.run([check_bin], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.splitlines() == ["%s: %s" % e for e in EXPECTED]
