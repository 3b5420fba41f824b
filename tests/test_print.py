"""The model text and histogram (colibri-patternmodeller -P / -H; colibri_print_model / colibri_histogram, csrc/print.hpp), without a device: the
"%.6g" formatter of csrc/fmt_g6.hpp against printf, a restatement of the row text and of the histogram from a model's flat arrays, checked
against the text the reference prints for the model files of tests/golden/views/, and the presence of the new entry points.
test_gpu_print.py holds the device to this restatement."""
import os
import subprocess

import numpy as np
import pytest

from test_coverage import category_of, load_case, tokens_of
from test_views import CASES, GOLD, ROOT, golden

CATEGORY_WORDS = {1: b"ngram", 2: b"skipgram", 3: b"flexgram"}
PRESET = {1: b"{|}", 2: b"{?}", 3: b"{*}", 4: b"{**}"}  # what a ClassDecoder holds before it loads a file


def read_classes(path):
    words = dict(PRESET)
    with open(path, "rb") as f:
        for line in f:
            k, _, w = line.rstrip(b"\n").partition(b"\t")
            if k:
                words[int(k)] = w
    return words


def g6(a, b):
    """what an ostream in its default state writes for a / (double)b: printf's %.6g, which Python's %g is (both round the exact binary value of
    the correctly rounded quotient); a division by zero gives inf, or x86-64's default NaN, which prints as -nan"""
    if b == 0:
        return b"inf" if a else b"-nan"
    return (b"%g" % (a / b))


def text_of(toks, words):
    """Pattern::tostring: one space between words, written only when the text so far is not empty; {?} for an id without a word"""
    out = b""
    for t in toks:
        if out:
            out += b" "
        out += words[t] if t in words else b"{?}"
    return out


def print_rows(words, arrays, tokens):
    """the rows of PatternModel::print for a model (key_off, key_bytes, counts | None, (ref_off, rs, rt) | None), in the order of the arrays"""
    key_off, key_bytes, counts, refs = arrays
    kb, off = bytes(bytearray(np.asarray(key_bytes, dtype=np.uint8).tolist())), [int(x) for x in key_off]
    npat = len(off) - 1
    if refs is not None:
        ro, rs, rt = ([int(x) for x in a] for a in refs)
    toks = [tokens_of(kb[off[j]:off[j + 1]]) for j in range(npat)]
    count = [int(counts[j]) if counts is not None else ro[j + 1] - ro[j] for j in range(npat)]
    total = {}
    for j, t in enumerate(toks):
        c, n = category_of(t), len(t)
        for g in {(c, 0)} | (set() if c == 3 else {(c, n)}):  # a flexgram is in its all-sizes group only
            total[g] = total.get(g, 0) + count[j]
    rows = []
    for j, t in enumerate(toks):
        c, n = category_of(t), len(t)
        gt = 0 if (c == 3 and n != 0) else total.get((c, n), 0) & 0xFFFFFFFF  # (unsigned int)totaloccurrencesingroup
        row = b"\t".join([text_of(t, words), b"%d" % count[j], b"%d" % (count[j] * n), g6(count[j] * n, tokens), CATEGORY_WORDS[c], b"%d" % n, g6(count[j], gt)])
        if refs is not None:
            row += b"\t" + b" ".join(b"%d:%d" % (rs[r], rt[r]) for r in range(ro[j], ro[j + 1]))
        rows.append(row + b"\n")
    return rows


def histogram_rows(arrays, category=0, size=0):
    """(distinct counts ascending, patterns of each) over the patterns of one (category, size) group, 0 = all"""
    key_off, key_bytes, counts, refs = arrays
    kb, off = bytes(bytearray(np.asarray(key_bytes, dtype=np.uint8).tolist())), [int(x) for x in key_off]
    hist = {}
    for j in range(len(off) - 1):
        t = tokens_of(kb[off[j]:off[j + 1]])
        if (category and category_of(t) != category) or (size and len(t) != size):
            continue
        c = int(counts[j]) if counts is not None else int(refs[0][j + 1]) - int(refs[0][j])
        hist[c] = hist.get(c, 0) + 1
    keys = sorted(hist)
    return np.array(keys, dtype=np.uint32), np.array([hist[k] for k in keys], dtype=np.uint64)


def histogram_text(pairs):
    counts, patterns = pairs
    return b"HISTOGRAM\n" + b"-" * 30 + b"\nOCCURRENCES\tPATTERNS\n" + b"".join(b"%d\t%d\n" % (int(c), int(p)) for c, p in zip(counts, patterns))


def case_arrays(case):
    indexed, tokens, types, key_off, key_bytes, counts, refs = load_case(case)
    return indexed, tokens, (key_off, key_bytes, None if indexed else counts, refs if indexed else None)


def test_formatter_against_printf(tmp_path):
    """csrc/fmt_g6.hpp, compiled for the host, against snprintf("%.6g"): every a <= 3b for b <= 1500, the exponent forms, exact decimal ties at the
    seventh digit and their neighbours, two million random pairs under 2^40 (tests/fmt_g6_check.cpp holds the cases)"""
    exe = tmp_path / "fmt_g6_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "colibri-core_amd", "csrc"), os.path.join(ROOT, "tests", "fmt_g6_check.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:]
    checked, mismatches = (int(x) for x in p.stdout.split()[1::2][-2:])
    assert mismatches == 0 and checked > 5_000_000, p.stdout[-500:]


def test_restatement_of_the_doubles():
    assert [g6(a, b) for a, b in ((0, 5), (1, 3), (9999995, 10 ** 7), (99999950, 10 ** 12), (1, 10 ** 5), (1234565, 10 ** 7), (10 ** 6, 1), (5, 0), (0, 0))] == \
        [b"0", b"0.333333", b"1", b"0.0001", b"1e-05", b"0.123456", b"1e+06", b"inf", b"-nan"]


@pytest.mark.parametrize("case", list(CASES))
def test_restatement_reproduces_the_reference_text(case):
    indexed, tokens, arrays = case_arrays(case)
    words = read_classes(os.path.join(GOLD, CASES[case][2]))
    want = golden(case, "print").split(b"\n")
    assert want[0] == b"PATTERN\tCOUNT\tTOKENS\tCOVERAGE\tCATEGORY\tSIZE\tFREQUENCY" + (b"\tREFERENCES" if indexed else b"")
    assert sorted(b"".join(print_rows(words, arrays, tokens)).split(b"\n")) == sorted(want[1:])
    assert histogram_text(histogram_rows(arrays)) == golden(case, "histogram")


def test_restatement_on_a_model_written_by_hand():
    """an empty first word leaves no space behind it, an id without a word prints {?}, a redefined class 3 prints its new word, a flexgram's
    frequency is a division by its missing per-size group, a pattern without references keeps its tab"""
    words = {5: b"", 6: b"b", 3: b"GAP", 4: b"{**}", 300: b"far"}
    keys = [b"\x05\x06", b"\x06\x05\x06", b"\x06\x03\x07", b"\x06\x04\x06", b"\xac\x02"]
    refs = [[(1, 0), (2, 3)], [], [(4294967295, 65535)], [(1, 1)], [(7, 0), (7, 1), (8, 0)]]
    key_off = np.cumsum([0] + [len(k) for k in keys]).astype(np.uint64)
    ref_off = np.cumsum([0] + [len(r) for r in refs]).astype(np.uint64)
    rs = np.array([s for r in refs for s, _ in r], dtype=np.uint32)
    rt = np.array([t for r in refs for _, t in r], dtype=np.uint16)
    arrays = (key_off, np.frombuffer(b"".join(keys), dtype=np.uint8), None, (ref_off, rs, rt))
    assert print_rows(words, arrays, 40) == [
        b"b\t2\t4\t0.1\tngram\t2\t1\t1:0 2:3\n",
        b"b  b\t0\t0\t0\tngram\t3\t-nan\t\n",
        b"b GAP {?}\t1\t3\t0.075\tskipgram\t3\t1\t4294967295:65535\n",
        b"b {**} b\t1\t3\t0.075\tflexgram\t3\tinf\t1:1\n",
        b"far\t3\t3\t0.075\tngram\t1\t1\t7:0 7:1 8:0\n",
    ]
    assert [a.tolist() for a in histogram_rows(arrays)] == [[0, 1, 2, 3], [1, 2, 1, 1]]
    assert [a.tolist() for a in histogram_rows(arrays, 1, 0)] == [[0, 2, 3], [1, 1, 1]]
    assert [a.tolist() for a in histogram_rows(arrays, 0, 3)] == [[0, 1], [1, 2]]


def test_the_library_and_the_python_face_have_the_print_calls():
    from colibri_amd import capi
    L = capi.load()
    for name in ("colibri_print_classes", "colibri_print_model", "colibri_print_model_resident", "colibri_print_info", "colibri_histogram", "colibri_histogram_resident",
                 "colibri_histogram_fetch"):
        assert name in capi.EXPORTED and hasattr(L, name)
    for method in ("print_model", "print_info", "histogram"):
        assert callable(getattr(capi.Context, method))
