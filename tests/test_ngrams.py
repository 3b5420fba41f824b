"""N-gram extraction (colibri-extractngrams; reference src/extractngrams.cpp).

CPU part: a restatement of the specification (`reference_ngrams` below), held to the real reference's stdout on every fixture case
(tests/golden/ngrams/, see the README there); the CLI's refusals that need no device; the two new names in the header and in capi.EXPORTED.
The GPU part (tests/test_gpu_ngrams.py) holds the device, the C++ face and the CLI against the fixtures and this restatement."""
import gzip
import json
import os
import re
import subprocess

import pytest

from conftest import GOLDEN, ROOT
from test_decode import read_classes

NGR = os.path.join(GOLDEN, "ngrams")
CLI = os.path.join(ROOT, "colibri-core_amd", "bin", "colibri-extractngrams")
CASES = json.load(open(os.path.join(NGR, "cases.json")))
IDS = [c["name"] for c in CASES]


def tokens_of(body):
    """the ids of a v2 payload, 0 for a 00; a last varint cut off by the end of the data is dropped (as colibri-classdecode drops it, §5d)"""
    ids, v, k = [], 0, 0
    for b in body:
        v |= (b & 127) << (7 * k)
        k += 1
        if b < 128:
            ids.append(v)
            v = k = 0
    return ids


def lines_of(body):
    """the lines of a payload as lists of ids (a last line without 00 ends with the data)"""
    lines, line = [], []
    for t in tokens_of(body) + [0]:
        if t:
            line.append(t)
        else:
            lines.append(line)
            line = []
    return lines


def text_of(cls, window, gap_words=False):
    """Pattern::tostring: a space before a token only when the text so far is not empty; {?} for an id without a word. gap_words: what the reference's
    PatternPointer::tostring makes of a window that holds a 04 among its first 31 tokens: the 03s among them print the word of class 4"""
    if gap_words and 4 in window[:31]:
        window = [4 if t == 3 else t for t in window[:31]] + window[31:]
    text = b""
    for t in window:
        if text:
            text += b" "
        text += cls.get(t, b"{?}")
    return text


def reference_ngrams(cls, data, n, keep_signature=False, stale_eof=False, gap_words=False):
    """what colibri-extractngrams -n <n> prints for the whole .colibri.dat `data` (A2 02 + payload) with the class map cls = {id: word bytes}.
    The three modes are the reference's own behaviour where this build departs from it. gap_words: see text_of. keep_signature: the two signature bytes are read as the first
    token of the first line. stale_eof: after a last line without 00 the read that meets the end of the file leaves the last byte in place, and
    that byte is taken as one more token (pattern.cpp:494-518, :550-562)."""
    assert n >= 1
    body = data if keep_signature else data[2:]
    if stale_eof and body and (body[-1] != 0 or (len(body) > 1 and body[-2] >= 128)):
        body += body[-1:]
    return b"".join(text_of(cls, line[i:i + n], gap_words) + b"\n" for line in lines_of(body) for i in range(len(line) - n + 1))


def golden(case):
    with gzip.open(os.path.join(NGR, case["stdout"]), "rb") as f:
        return f.read()


def want_of(case):
    """what this build prints for a case: the golden; for a case that records a departure the golden without the reference's one extra row (the first
    row: the signature read as a token; the last row: the stale byte after a last line without 00), or, where rows differ (03 beside 04), the restatement"""
    want = golden(case)
    if case["departure"] == "gaps":
        return reference_ngrams(*case_inputs(case), case["n"])
    if case["departure"] == "signature":
        return want[want.index(b"\n") + 1:]
    if case["departure"] == "eof":
        return want[:want.rindex(b"\n", 0, -1) + 1]
    return want


def case_inputs(case):
    cls = read_classes(open(os.path.join(GOLDEN, case["classes"]), "rb").read())
    data = open(os.path.join(GOLDEN, case["data"]), "rb").read()
    assert data[:2] == b"\xa2\x02"
    return cls, data


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restatement_matches_the_reference(case):
    cls, data = case_inputs(case)
    want = golden(case)
    assert len(want) == case["stdout_bytes"] and want.count(b"\n") == case["rows"]
    assert reference_ngrams(cls, data, case["n"], keep_signature=case["departure"] == "signature", stale_eof=case["departure"] == "eof", gap_words=case["departure"] == "gaps") == want


def test_fixtures_cover_the_issue():
    rows = {c["name"]: c["rows"] for c in CASES}
    assert rows["phrases15k_n1"] == 15000 and rows["phrases15k_n3"] == 13486 and rows["phrases15k_n5"] == 11972
    assert rows["zipf_n2"] == 4625 and rows["apology_n4"] == 19746 and rows["apology.t3U_n40"] == 4258
    assert rows["hamlet.v2_n3"] == 274 and rows["hamlet.v2_n3_signature"] == 275
    with_sig, without = (golden(next(c for c in CASES if c["name"] == k)) for k in ("hamlet.v2_n3_signature", "hamlet.v2_n3"))
    assert with_sig.split(b"\n")[0] == b"{?} To be"  # the signature bytes A2 02 read as the token 290: the one row this build does not print
    assert with_sig == b"{?} To be\n" + without  # (on the file without its first two bytes: the other 274 rows, unchanged)
    edge = open(os.path.join(NGR, "edge.colibri.dat"), "rb").read()
    assert edge[-1] < 128 and edge[-1] != 0  # a whole last token, no final 00
    longest = max(len(line) for line in lines_of(edge[2:]))
    assert {f"edge_n{k}" for k in (1, 2, 3, longest, longest + 1)} <= set(rows) and rows[f"edge_n{longest}"] == 1 and rows[f"edge_n{longest + 1}"] == 0
    e2 = golden(next(c for c in CASES if c["name"] == "edge_n2")).split(b"\n")
    for row in (b"{|} {?}", b"{?} SKIP-override", b"{**} {**}", b"eight\r ", b"ten"):
        assert row in e2
    assert all(not c["stderr"] for c in CASES if c["departure"] != "eof")
    assert not any(3 in line and 4 in line for c in CASES if c["departure"] != "gaps" for line in lines_of(case_inputs(c)[1][2:]))  # (only the gaps cases)
    gaps = next(c for c in CASES if c["name"] == "gaps_n2")
    assert golden(gaps).split(b"\n")[2] == b"{**} {**}" and want_of(gaps).split(b"\n")[2] == b"SKIP-override {**}"  # tokens 03 04
    eof, n1 = (golden(next(c for c in CASES if c["name"] == k)) for k in ("edge_n1_eof", "edge_n1"))
    assert eof == n1 + b"SIX-again\n"  # the stale byte 06 read as a token: the other row this build does not print


def run(args, **kw):
    if not os.path.exists(CLI):
        pytest.fail(f"{CLI} is not built (python -c 'import __graft_entry__ as g; g.build()')")
    return subprocess.run([CLI] + args, capture_output=True, timeout=120, **kw)


HAMLET = [os.path.join(GOLDEN, "hamlet.v2.colibri.dat")]
CLS = ["-c", os.path.join(GOLDEN, "hamlet.colibri.cls")]


@pytest.mark.parametrize("n", ["0", "-1", "-2147483649"])
def test_cli_refuses_n_below_one(n):
    r = run(CLS + ["-n", n] + HAMLET)
    assert r.returncode == 2 and r.stdout == b""
    assert b"ERROR: the n-gram size (-n) must be between 1 and 2147483647" in r.stderr


def test_cli_without_a_class_file_prints_the_references_message_and_usage():
    r = run(["-n", "3"] + HAMLET)
    assert r.returncode == 2 and r.stdout == b""
    lines = r.stderr.decode().splitlines()
    assert lines[0] == "ERROR: No class file specified! (-c)"
    assert lines[1] == "Syntax: colibri-extractngrams -n [size] -c classfile datafile datafile2 ..."


def test_cli_refuses_an_unknown_option():
    r = run(["-x"] + CLS + HAMLET)
    assert r.returncode == 2 and r.stdout == b""  # (the reference abort()s)
    assert b"ERROR: Unknown option: -x" in r.stderr


def test_cli_help_and_no_data_file():
    r = run(["-h"])
    assert r.returncode == 0 and b"Syntax: colibri-extractngrams" in r.stderr
    r = run(CLS)
    assert r.returncode == 0 and r.stdout == b"" and r.stderr == b""


def test_cli_missing_and_empty_data_file(tmp_path):
    r = run(CLS + [str(tmp_path / "none.colibri.dat")])
    assert r.returncode == 1 and r.stdout == b""
    assert b"ERROR: Supplied data file can not be opened. Check whether it exists and whether you have proper permissions..." in r.stderr
    empty = tmp_path / "empty.colibri.dat"
    empty.write_bytes(b"")
    r = run(CLS + [str(empty), str(empty)])
    assert r.returncode == 0 and r.stdout == b"" and r.stderr == b""


def test_cli_refuses_version_1_data_and_plain_text(tmp_path):
    for data in (os.path.join(GOLDEN, "hamlet.v1.colibri.dat"), os.path.join(GOLDEN, "decode", "markers.v1.colibri.dat")):
        r = run(CLS + [data])
        assert r.returncode == 1 and r.stdout == b""
        assert b"ERROR: Supplied data file is not version 2 Colibri data" in r.stderr
    headed = tmp_path / "headed.v1.colibri.dat"
    headed.write_bytes(b"\xa2\x01\x01\x06\x00")
    r = run(CLS + [str(headed)])
    assert r.returncode == 1 and b"ERROR: Supplied data file is not version 2 Colibri data" in r.stderr
    r = run(CLS + [os.path.join(GOLDEN, "classenc", "apology.txt")])
    assert r.returncode == 1 and r.stdout == b""
    assert b"ERROR: Supplied data file is not a valid Colibri Data file, did you pass plain-text instead perhaps?..." in r.stderr


def test_header_and_exported_list_have_the_two_functions():
    from colibri_amd import capi
    header = open(os.path.join(ROOT, "include", "colibri_hip.h")).read()
    assert re.search(r"^int colibri_ngrams\(colibri_ctx\* ctx, uint32_t n, colibri_decode_sink sink, void\* user, uint64_t\* outbytes, uint64_t\* nngrams\);", header, re.M)
    assert re.search(r"^int colibri_ngrams_info\(const colibri_ctx\* ctx, uint64_t\* windows, uint64_t\* staging_bytes, uint64_t\* scratch_bytes\);", header, re.M)
    assert {"colibri_ngrams", "colibri_ngrams_info"} <= set(capi.EXPORTED)
    assert re.search(r"#define COLIBRI_ABI_VERSION\s+4\b", header)
    L = capi.load()  # (dlopen needs no device)
    assert L.colibri_ngrams and L.colibri_ngrams_info
    assert hasattr(capi.Context, "ngrams") and hasattr(capi.Context, "ngrams_info")
