"""The connection lines of the trace audit's report formatter
(host/zkgpu_audit_format.hpp) as plain host code under the host sanitizers:
tests/cpp/conn_format_check.cpp is built with -fsanitize=address,undefined and
runs as a child process over connection reports of exact shape (full lists,
counts past the lists, foreign only, a label table shorter than the indices,
no report).  CPU only."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD = "trace audit: 2^10 = 1024 rows, 0 plookup(s), 3 grand product(s): NOT clean"
TAIL = "constraint check: every identity holds on the 2^10 = 1024 rows"
Z = ("calculateZ: grand product %d does not close (%d of 3 do not): 2 value(s) of num unmatched, the first at row 28 "
     "(1 in num, 0 in den); 2 value(s) of den unmatched, the first at row 28 (0 in num, 1 in den)")
C = "  connection: "


@pytest.fixture(scope="module")
def sections(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("conn_format_check") / "conn_format_check")
    subprocess.check_call(
        # (the sanitizer runtimes linked statically: the program needs no place in a preload list)
        ["g++", "-O1", "-g", "-std=c++20", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         "-static-libasan", "-static-libubsan", "-o", out, os.path.join(ROOT, "tests/cpp/conn_format_check.cpp")])
    r = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", (r.stdout[-2000:], r.stderr[-4000:])
    secs, name = {}, None
    for line in r.stdout.splitlines():
        if line.startswith("== "):
            name = line[3:]
            secs[name] = []
        else:
            secs[name].append(line)
    return secs


def test_no_report_prints_what_it_printed_before(sections):
    assert sections["undeclared"] == [HEAD, Z % (2, 1), TAIL]
    assert sections["not_ran"] == sections["undeclared"]
    assert sections["short_reports"] == [HEAD, Z % (0, 2), Z % (2, 2), TAIL]


def test_one_wrong_cell_is_two_links(sections):
    assert sections["one_cell"] == [
        HEAD, Z % (2, 1),
        C + "2 cell(s) differ from the cell they are wired to; pols[0] row 28 (= 6) is wired to pols[1] row 37 (= 5)",
        C + "pols[1] row 37 (= 5) is wired to pols[0] row 28 (= 6)", TAIL]
    s = sections["one_cell_labels"]
    assert s[2] == (C + "2 cell(s) differ from the cell they are wired to; pols[0] (cm1 column 4) row 28 (= 6) is "
                    "wired to pols[1] (cm1 column 9) row 37 (= 5)")
    assert s[3] == C + "pols[1] (cm1 column 9) row 37 (= 5) is wired to pols[0] (cm1 column 4) row 28 (= 6)"
    # a label table shorter than the indices: the plain name, nothing read past an end
    assert sections["short_labels"][3] == C + "pols[1] row 37 (= 5) is wired to pols[0] (cm1 column 4) row 28 (= 6)"
    assert sections["short_table"] == sections["one_cell"]


def test_full_lists_say_what_they_leave_out(sections):
    s = sections["full_lists"]
    assert s[:3] == [HEAD, Z % (0, 2), Z % (2, 2)] and s[-1] == TAIL and len(s) == 3 + 17 + 17 + 1 + 1
    assert s[3] == (C + "40 cell(s) differ from the cell they are wired to; pols[0] row 0 (= 100) is wired to pols[1] "
                    "row 1 (= 200)")
    assert s[4:19] == [C + "pols[%d] row %d (= %d) is wired to pols[%d] row %d (= %d)"
                       % (e // 8, 10 * e, 100 + e, 1 - e // 8, 10 * e + 1, 200 + e) for e in range(1, 16)]
    assert s[19] == C + "and 24 more"
    assert s[20] == (C + "17 cell(s) of S hold no cell's identity (a damaged or mismatched constant file); S of pols[1] "
                     "row 0 holds 0")
    assert s[21:36] == [C + "S of pols[1] row %d holds %d" % (5 * e, e) for e in range(1, 16)]
    assert s[36] == C + "and 1 more"
    assert s[37] == C + "3 cell(s) are named by no S value: S is not a permutation of the cells"
    assert sections["counts_only"][3:5] == [
        C + "5 cell(s) differ from the cell they are wired to",
        C + "1 cell(s) of S hold no cell's identity (a damaged or mismatched constant file)"]


def test_foreign_untargeted_and_clean(sections):
    assert sections["foreign_only"] == [
        HEAD, Z % (1, 1),
        C + "1 cell(s) of S hold no cell's identity (a damaged or mismatched constant file); S of pols[1] row 1023 "
        "holds 0",
        C + "1 cell(s) are named by no S value: S is not a permutation of the cells", TAIL]
    assert sections["untargeted_only"] == [
        HEAD, Z % (1, 1), C + "1 cell(s) are named by no S value: S is not a permutation of the cells", TAIL]
    assert sections["clean_connection"][2] == (
        C + "every cell holds the value of the cell it is wired to and S names every cell once; the wiring is not "
        "what keeps the product open")
