"""A model queried with new text (colibri-patternmodeller -q / --queryfile; PatternModel::getpatterns / query; ClassEncoder::encodestring).

CPU part: a plain restatement of the specification (reference src/patternmodeller.cpp:160-231, include/patternmodel.h:2272-2285,
src/classencoder.cpp:369-447), held byte for byte to what the reference's own colibri-patternmodeller wrote for -Q and -q
(tests/golden/query/, see the README there); the C++ face's encodestring / buildpattern; the CLI on the host route. The GPU part
(tests/test_gpu_query.py) holds the device against this restatement."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from test_cooc import CLI, COOC, key_tokens
from test_coverage import tokens_of
from test_gpu_coverage import varint
from test_host_face import parse_model
from test_print import print_rows, read_classes, text_of

QUERY = os.path.join(GOLDEN, "query")
MISS = 0xFFFFFFFF
# golden case -> (model file under tests/golden, class file, query file); the -Q output is <case>.Q.txt, the -q output <case>.q.txt
CASES = {
    "hamlet.v2.i": ("cooc/hamlet.v2.i.colibri.patternmodel", "hamlet.colibri.cls", "hamlet.lines.txt"),
    "hamlet.v2.is": ("cooc/hamlet.v2.is.colibri.patternmodel", "hamlet.colibri.cls", "hamlet.lines.txt"),
    "edge.i": ("cooc/edge.i.colibri.patternmodel", "synthetic.colibri.cls", "edge.lines.txt"),
    "edge.is": ("cooc/edge.is.colibri.patternmodel", "synthetic.colibri.cls", "edge.lines.txt"),
    "hamlet.u": ("compare/hamlet.v2.20.us.colibri.patternmodel", "hamlet.colibri.cls", "hamlet.lines.txt"),
    "hamlet.m2": ("query/hamlet.m2.colibri.patternmodel", "hamlet.colibri.cls", "hamlet.lines.txt"),
}
# the -q patterns of every case: its query file's lines that are neither blank nor the mode switch
MARKERS = {b"{*}": [3], b"{**}": [4], b"{?}": [2]}


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def encodestring(line, classes, allowunknown=True):
    """ClassEncoder::encodestring(line, buffer, allowunknown): the tokens of a line as key bytes, one entry per token. Words are cut at
    single spaces, trimmed of " \\t\\n\\r\\b", empty ones dropped; {*} {**} {?} are the classes 3, 4, 2, {*N*} is N times class 3; a word
    the class file does not have is class 2, or, when unknown words are not allowed, an error."""
    out = []
    for word in line.split(b" "):
        word = word.strip(b" \t\n\r\b")
        if not word:
            continue
        if word in MARKERS:
            out.append(varint(MARKERS[word][0]))
        elif len(word) >= 4 and word.startswith(b"{*") and word.endswith(b"*}"):
            digits = word[2:-2].lstrip(b" \t\n\r\v\f")  # atoi: leading blanks, a sign, digits
            sign, k = (-1 if digits[:1] == b"-" else 1), (1 if digits[:1] in (b"-", b"+") else 0)
            n = 0
            while k < len(digits) and digits[k:k + 1].isdigit():
                n, k = n * 10 + int(digits[k:k + 1]), k + 1
            out.extend([varint(3)] * max(0, sign * n))
        elif word in classes or allowunknown:
            out.append(varint(classes.get(word, 2)))
        else:
            raise KeyError(word)
    return out


def read_query(text):
    """the lines of a query file as the batch sees them: [(token list | None, exact)], None for a line that prints nothing and is only counted
    (blank, or the mode switch X)"""
    out, exact = [], False
    lines = text.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()  # (the text ends in a newline: no line after it)
    for line in lines:
        if line == b"X":
            exact = not exact
            out.append((None, exact))
        elif line == b"":
            out.append((None, exact))
        else:
            out.append((line, exact))
    return out


def query_rows(counts, lines, exact, minlength, maxlength):
    """[(line, token, key | None)] in the defined order: per line the whole-line row when the model has the line (exact mode: always, None
    for a miss), then n ascending, then tokens ascending"""
    rows = []
    for s, toks in enumerate(lines):
        whole = b"".join(toks)
        if exact[s]:
            rows.append((s, 0, whole if toks and whole in counts else None))
            continue
        if toks and whole in counts:
            rows.append((s, 0, whole))
        for n in range(max(1, minlength), min(maxlength, len(toks)) + 1):
            for i in range(len(toks) - n + 1):
                w = b"".join(toks[i:i + n])
                if w in counts:
                    rows.append((s, i, w))
    return rows


def model_arrays(counts, refs=None):
    """(key_off, key_bytes, counts | None, (ref_off, rs, rt) | None) in the order of `counts`; an indexed model's counts are its references"""
    keys = list(counts)
    key_off = np.cumsum([0] + [len(k) for k in keys]).astype(np.uint64)
    key_bytes = np.frombuffer(b"".join(keys) + b"\0", dtype=np.uint8)[:-1]
    if refs is None:
        return key_off, key_bytes, np.array([counts[k] for k in keys], dtype=np.uint32), None
    ref_off = np.cumsum([0] + [len(refs[k]) for k in keys]).astype(np.uint64)
    rs = np.array([s for k in keys for s, _ in refs[k]], dtype=np.uint32)
    rt = np.array([t for k in keys for _, t in refs[k]], dtype=np.uint16)
    return key_off, key_bytes, None, (ref_off, rs, rt)


def query_text(rows, lines, exact, counts, arrays, words, tokens, first_line=1):
    """the text of the rows: "L:i\\t" + the print() row in extensive mode; the print() row, or the NOT FOUND line, in exact mode"""
    printed = dict(zip(counts, print_rows(words, arrays, tokens)))
    out = []
    for s, i, k in rows:
        if k is None:
            out.append(b'PATTERN "' + text_of(tokens_of(b"".join(lines[s])), words) + b'" NOT FOUND IN MODEL\n')
        else:
            out.append((b"" if exact[s] else b"%d:%d\t" % (first_line + s, i)) + printed[k])
    return b"".join(out)


def model_lengths(counts):
    lens = [len(key_tokens(k)) for k in counts]
    return (min(lens), max(lens)) if lens else (1, 0)


def batch(text, classes):
    """a query file as the device takes it: (token lists, exact flags); a line that prints nothing is an empty line of extensive mode"""
    lines, exact = [], []
    for line, ex in read_query(text):
        toks = None if line is None else encodestring(line, classes)
        lines.append(toks or [])
        exact.append(bool(ex) and line is not None)
    return lines, exact


def classes_of(words):
    return {w: k for k, w in words.items() if k > 4}


def load_case(case):
    model, cls, _ = CASES[case]
    mtype, tokens, _, counts, refs = parse_model(os.path.join(GOLDEN, model))
    words = read_classes(os.path.join(GOLDEN, cls))
    return counts, (refs if mtype == 20 else None), tokens, words


def expected_text(case, text):
    counts, refs, tokens, words = load_case(case)
    lines, exact = batch(text, classes_of(words))
    mn, mx = model_lengths(counts)
    rows = query_rows(counts, lines, exact, mn, mx)
    # (the reference's query prints the row of the plain model, without the REFERENCES column, for an indexed model too: DESIGN.md §6)
    return query_text(rows, lines, exact, counts, model_arrays(counts), words, tokens)


def cli(args, stdin=None, ok=0, **env):
    p = subprocess.run([CLI] + args, input=stdin, capture_output=True, env={**os.environ, **env}, timeout=300)
    assert p.returncode == ok, p.stderr.decode()[-2000:]
    return p.stdout, p.stderr.decode()


def case_files(case):
    model, cls, lines = CASES[case]
    return os.path.join(GOLDEN, model), os.path.join(GOLDEN, cls), os.path.join(QUERY, lines)


def q_patterns(text):
    return [l for l in text.split(b"\n") if l.strip(b" \t\r") and l != b"X"]


# ---- the restatement against the reference --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_restatement_equals_the_references_queryfile_output(case):
    text = open(case_files(case)[2], "rb").read()
    assert expected_text(case, text) == open(os.path.join(QUERY, case + ".Q.txt"), "rb").read()


@pytest.mark.parametrize("case", list(CASES))
def test_restatement_equals_the_references_q_output(case):
    pats = q_patterns(open(case_files(case)[2], "rb").read())
    assert expected_text(case, b"X\n" + b"\n".join(pats) + b"\n") == open(os.path.join(QUERY, case + ".q.txt"), "rb").read()


def test_the_query_files_hold_the_cases_they_are_for():
    for name, cls in (("hamlet.lines.txt", "hamlet.colibri.cls"), ("edge.lines.txt", "synthetic.colibri.cls")):
        text = open(os.path.join(QUERY, name), "rb").read()
        classes = classes_of(read_classes(os.path.join(GOLDEN, cls)))
        entries = read_query(text)
        toks = [(encodestring(l, classes), ex) for l, ex in entries if l is not None]
        assert any(l == b"" for l in text.split(b"\n")[:-1]) and text.count(b"\nX\n") >= 2
        assert any(len(t) == 1 for t, _ in toks) and any(len(t) > 8 for t, _ in toks)
        assert any(varint(2) in t for t, _ in toks) and any(varint(3) in t for t, _ in toks)
        assert any(ex for _, ex in toks) and any(not ex for _, ex in toks)


# ---- the CLI on the host route ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_cli_queryfile_on_the_host_route(case):
    model, cls, lines = case_files(case)
    want = open(os.path.join(QUERY, case + ".Q.txt"), "rb").read()
    out, err = cli(["-i", model, "-c", cls, "--queryfile", lines] + (["-u"] if case in ("hamlet.u", "hamlet.m2") else []), COLIBRI_QUERY="host")
    assert out == want and "on the device" not in err
    out, _ = cli(["-i", model, "-c", cls, "--queryfile", "-"] + (["-u"] if case in ("hamlet.u", "hamlet.m2") else []), stdin=open(lines, "rb").read(), COLIBRI_QUERY="host")
    assert out == want


@pytest.mark.parametrize("case", list(CASES))
def test_cli_q_on_the_host_route(case):
    model, cls, lines = case_files(case)
    pats = q_patterns(open(lines, "rb").read())
    args = ["-i", model, "-c", cls] + (["-u"] if case in ("hamlet.u", "hamlet.m2") else [])
    for p in pats:
        args += ["-q", p.decode()]
    out, err = cli(args, COLIBRI_QUERY="host")
    assert out == open(os.path.join(QUERY, case + ".q.txt"), "rb").read()
    assert f"Processing {len(pats)} queries" in err


def test_cli_auto_stays_on_the_host():
    model, cls, lines = case_files("hamlet.v2.i")
    out, err = cli(["-i", model, "-c", cls, "--queryfile", lines])
    assert out == open(os.path.join(QUERY, "hamlet.v2.i.Q.txt"), "rb").read() and "on the device" not in err


def test_cli_interactive_Q_is_still_refused():
    model, cls, _ = case_files("hamlet.v2.i")
    p = subprocess.run([CLI, "-i", model, "-c", cls, "-Q"], capture_output=True, input=b"", timeout=60)
    assert p.returncode == 2 and b"not part of the MI355X-accelerated build" in p.stderr


def test_cli_query_needs_a_class_file():
    model, _, lines = case_files("hamlet.v2.i")
    for args in (["-q", "to be"], ["--queryfile", lines]):
        p = subprocess.run([CLI, "-i", model] + args, capture_output=True, timeout=60)
        assert p.returncode == 2 and b"-c" in p.stderr


def test_cli_relations_of_queries_stay_refused():
    model, cls, _ = case_files("hamlet.v2.i")
    for flag in ("-g", "--leftcooc", "--rightcooc"):
        p = subprocess.run([CLI, "-i", model, "-c", cls, "-q", "to be", flag], capture_output=True, timeout=60)
        assert p.returncode == 2 and b"not part of the MI355X-accelerated build" in p.stderr, flag


# ---- encodestring / buildpattern of the C++ face -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def encode_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("query") / "query_encode_check")
    host = os.path.join(ROOT, "colibri-core_amd", "host")
    lib = os.path.join(ROOT, "colibri-core_amd", "lib")  # (the face's archive and the device layer it calls, as the CLI links them)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(host, "include"), "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "query_encode_check.cpp"), os.path.join(lib, "libcolibri_amd_host.a"), "-L" + lib, "-lcolibri_hip",
                           "-Wl,-rpath," + lib, "-L/opt/rocm/lib", "-lrccl", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib", "-lpthread", "-o", exe])
    return exe


@pytest.mark.parametrize("name,cls", [("hamlet.lines.txt", "hamlet.colibri.cls"), ("edge.lines.txt", "synthetic.colibri.cls")])
def test_encodestring_and_buildpattern_of_the_host_face(encode_check, name, cls):
    """every line of the query files through ClassEncoder::encodestring and buildpattern (allowunknown): the key bytes and token counts of the
    restatement, whose rows the goldens confirm; an unknown word without allowunknown throws"""
    path = os.path.join(QUERY, name)
    out = subprocess.run([encode_check, os.path.join(GOLDEN, cls), path], capture_output=True, timeout=60, check=True).stdout.split(b"\n")
    classes = classes_of(read_classes(os.path.join(GOLDEN, cls)))
    lines = open(path, "rb").read().split(b"\n")[:-1]
    want = []
    for l in lines:
        toks = encodestring(l, classes)
        try:
            encodestring(l, classes, allowunknown=False)
            strict = b"ok"
        except KeyError:
            strict = b"throws"
        want.append(b"%d %s %s %s" % (len(toks), b"".join(toks).hex().encode() or b"-", b"".join(toks).hex().encode() or b"-", strict))
    assert out[:-1] == want
