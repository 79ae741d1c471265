"""The trace audit's report formatter (host/zkgpu_audit_format.hpp) as plain
host code under the host sanitizers: tests/cpp/audit_format_check.cpp is built
with -fsanitize=address,undefined and runs as a child process over reports of
exact shape (every list full, counts past the lists, context tables shorter
than the indices).  CPU only."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD = "trace audit: 2^10 = 1024 rows, 2 plookup(s), 5 grand product(s): "
NOT_RUN = ("constraint check: not run: a plookup missed, so its h1 / h2 columns are meaningless and the combination "
           "would fail on almost every row; fix the plookup(s) and audit again")
PERM = ("calculateZ: grand product 2 does not close (2 of 5 do not): 1 value(s) of num unmatched, the first at row 86 "
        "(1 in num, 0 in den); 1 value(s) of den unmatched, the first at row 77 (0 in num, 1 in den); grand product 2 "
        "is permutation check 0 (peCtx[0])")


@pytest.fixture(scope="module")
def sections(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("audit_format_check") / "audit_format_check")
    subprocess.check_call(
        # (the sanitizer runtimes linked statically: the program needs no place in a preload list)
        ["g++", "-O1", "-g", "-std=c++20", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         "-static-libasan", "-static-libubsan", "-o", out, os.path.join(ROOT, "tests/cpp/audit_format_check.cpp")])
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


def test_clean_and_refused(sections):
    assert sections["clean"] == [HEAD + "clean", "constraint check: every identity holds on the 2^10 = 1024 rows"]
    assert sections["identities_refused"] == [
        HEAD + "NOT clean", "constraint check: not run: step42ns: operand 3: row shift 1 is no multiple of 2"]
    assert sections["identities_no_reason"][1] == "constraint check: not run: unknown reason"


def test_full_lists_say_what_they_leave_out(sections):
    s = sections["full_lists"]
    assert s[0] == "trace audit: 2^10 = 1024 rows, 11 plookup(s), 12 grand product(s): NOT clean"
    assert s[1] == ("Polinomial::calculateH1H2() Number not included: w=0 plookup_number=1: 100 row(s) of f hold 40 "
                    "value(s) the table does not")
    assert s[2:18] == ["  plookup 1: the value of row %d on %d row(s)" % (7 * j, j + 1) for j in range(16)]
    assert s[18] == "  plookup 1: and 24 more value(s)"
    assert sum(l.startswith("Polinomial::calculateH1H2()") for l in s) == 8
    assert "and 2 more plookup(s) with misses (10 of 11)" in s
    z = [l for l in s if l.startswith("calculateZ: ")]
    assert len(z) == 8 and all("(9 of 12 do not)" in l for l in z)
    assert z[3] == ("calculateZ: grand product 5 does not close (9 of 12 do not); the comparison of its num and den "
                    "columns was skipped")
    assert z[0].endswith(": no value of num unmatched; 2 value(s) of den unmatched, the first at row 9 (0 in num, 1 "
                         "in den)")
    assert s[-3:] == ["and 1 more open grand product(s)",
                      "(a plookup that missed leaves its own grand product open: its h1 / h2 were zeroed)", NOT_RUN]


def test_contexts_and_names(sections):
    s = sections["labels_plookup_missed"]
    assert s[1] == ("Polinomial::calculateH1H2() Number not included: w=17 plookup_number=1: plookup 1 (puCtx[1]): 2 "
                    "row(s) of f hold 1 value(s) the table does not")
    assert s[3].endswith("; grand product 1 is plookup 1 (puCtx[1]); it follows from the misses of plookup 1 (its h1 / "
                         "h2 were zeroed)")
    assert s[4] == PERM and s[5] == NOT_RUN and len(s) == 6
    n = sections["named_rows"]
    assert n[2] == "constraint check: 20 of the 2^10 = 1024 rows of the trace break the AIR; the first is row 0"
    assert n[3:6] == ["  row 0: failing terms: 4", "  row 3: failing terms: 0 1 2 3 4 5 6 7 and 1 more",
                      "  row 6: no live term fails"]
    assert len(n) == 3 + 16 + 1 and n[-1] == "  and 4 more row(s)"
    assert sections["rows_only"][3:19] == ["  row %d" % (3 * j) for j in range(16)]
    t = sections["short_tables"]
    assert t[1].startswith("Polinomial::calculateH1H2() Number not included: w=3 plookup_number=7: 1 row(s)")
    assert "is permutation check" not in t[3] and t[7] == "  row 6"
