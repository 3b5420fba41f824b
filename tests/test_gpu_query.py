"""A model queried with new text on the device (colibri_query / colibri_query_resident / colibri_query_text; colibri-patternmodeller -q /
--queryfile under COLIBRI_QUERY=device), against the restatement of test_query.py: the arrays exactly, order included, and the text byte for
byte."""
import os
import random

import numpy as np
import pytest

from conftest import GOLDEN
from test_cooc import COOC, sentences
from test_gpu_coverage import varint
from test_host_face import parse_model
from test_oracle import read_payload
from test_print import read_classes
from test_query import CASES, MISS, QUERY, batch, case_files, classes_of, cli, load_case, model_arrays, model_lengths, q_patterns, query_rows, query_text
from test_rindex import cls_for

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from colibri_amd import capi
    with capi.Context(0) as c:
        yield c


def payload_of(lines):
    return b"".join(b"".join(t) + b"\x00" for t in lines)


def rows_of(keys, fetched, nlines):
    line_off, token, pattern = fetched
    lo = [int(x) for x in line_off]
    assert len(lo) == nlines + 1 and lo[0] == 0 and lo[-1] == len(token) == len(pattern)
    return [(s, int(token[r]), None if int(pattern[r]) == MISS else keys[int(pattern[r])]) for s in range(nlines) for r in range(lo[s], lo[s + 1])]


def check(ctx, counts, lines, exact=None, minlength=None, maxlength=None, refs=None, first_line=1, words=None, tokens=1000):
    """one uploaded query against the restatement: the rows, and with `words` the text"""
    keys = list(counts)
    arrays = model_arrays(counts, refs)
    mn, mx = model_lengths(counts)
    minlength, maxlength = (mn if minlength is None else minlength), (mx if maxlength is None else maxlength)
    ex = [False] * len(lines) if exact is None else exact
    got = rows_of(keys, ctx.query(payload_of(lines), arrays[0], arrays[1], arrays[2], arrays[3], exact=None if exact is None else np.array(ex, dtype=np.uint8),
                                  minlength=minlength, maxlength=maxlength, first_line=first_line), len(lines))
    want = query_rows(counts, lines, ex, minlength, maxlength)
    assert got == want
    if words is not None:
        assert ctx.query_text(words, tokens) == query_text(want, lines, ex, counts, arrays, words, tokens, first_line)
    return want


def fixture(corpus, kind):
    path = os.path.join(COOC, f"{corpus}.{kind}.colibri.patternmodel") if kind != "u" else os.path.join(GOLDEN, "compare", f"{corpus}.20.us.colibri.patternmodel")
    mtype, tokens, _, counts, refs = parse_model(path)
    return counts, (refs if mtype == 20 else None), tokens


# ---- the fixture models -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("corpus,kind", [("hamlet.v2", "i"), ("hamlet.v2", "is"), ("hamlet.v2", "u"), ("edge", "i"), ("edge", "is")])
def test_uploaded_model_equals_the_restatement(ctx, corpus, kind):
    counts, refs, tokens = fixture(corpus, kind)
    words = read_classes(cls_for(corpus))
    other = "edge" if corpus == "hamlet.v2" else "hamlet.v2"
    own, others = sentences(read_payload(corpus)), sentences(read_payload(other))
    rows = check(ctx, counts, own, refs=refs, words=words, tokens=tokens)
    assert rows
    check(ctx, counts, others[:300], refs=refs, words=words, tokens=tokens, first_line=7)
    exact = [s % 3 == 0 for s in range(len(own))]
    check(ctx, counts, own, exact=exact, refs=refs, words=words, tokens=tokens)


@pytest.mark.parametrize("case", list(CASES))
def test_golden_query_files(ctx, case):
    counts, refs, tokens, words = load_case(case)
    text = open(case_files(case)[2], "rb").read()
    lines, exact = batch(text, classes_of(words))
    check(ctx, counts, lines, exact=exact, refs=refs, words=words, tokens=tokens)  # (with the references of an indexed model in its rows)
    check(ctx, counts, lines, exact=exact, words=words, tokens=tokens)             # (and as the reference prints them: the counts alone)
    assert ctx.query_text(words, tokens) == open(os.path.join(QUERY, case + ".Q.txt"), "rb").read()


@pytest.mark.parametrize("corpus,indexed,skipgrams", [("hamlet.v2", 1, 1), ("hamlet.v2", 1, 0), ("hamlet.v2", 0, 0), ("edge", 1, 1), ("edge", 0, 0)])
def test_resident_model_equals_the_restatement_and_is_left_alone(ctx, corpus, indexed, skipgrams):
    payload = read_payload(corpus)
    ctx.upload(payload)
    ctx.train(mintokens=2, maxlength=4, indexed=indexed, doskipgrams=skipgrams)
    counts, _ = ctx.export_dict()
    flat = lambda arrs: [np.array(a) for a in arrs[:3]] + [np.array(a) for a in (arrs[3] or ())]
    before = flat(ctx.export_arrays())
    rindex_before = [np.array(a).copy() for a in ctx.reverse_index(resident=True)]
    key_off, key_bytes, cnt, refs = ctx.export_arrays()
    kb, off = key_bytes.tobytes(), key_off.tolist()
    keys = [kb[off[j]:off[j + 1]] for j in range(len(off) - 1)]
    words = read_classes(cls_for(corpus))
    other = sentences(read_payload("edge" if corpus == "hamlet.v2" else "hamlet.v2"))[:200]
    mn, mx = model_lengths(counts)
    for lines, exact in ((sentences(payload), None), (other, [s % 2 == 1 for s in range(len(other))])):
        ex = exact or [False] * len(lines)
        got = rows_of(keys, ctx.query(payload_of(lines), resident=True, exact=None if exact is None else np.array(ex, dtype=np.uint8), minlength=mn, maxlength=mx), len(lines))
        want = query_rows(counts, lines, ex, mn, mx)
        assert got == want
        arrays = (key_off, key_bytes, None if indexed else cnt, refs if indexed else None)
        assert ctx.query_text(words, 12345) == query_text(want, lines, ex, dict.fromkeys(keys), arrays, words, 12345)
    after = flat(ctx.export_arrays())
    assert len(before) == len(after) and all(np.array_equal(a, b) for a, b in zip(before, after))
    for a, b in zip(rindex_before, ctx.reverse_index(resident=True)):
        assert np.array_equal(a, b)


# ---- size edges: a tiny model, synthetic lines ------------------------------------------------------------------------------------------------------
A, B, C = varint(5), varint(300), varint(20000)  # tokens of 1, 2 and 3 bytes
TINY = {A: 3, B: 2, A + A: 4, A + B: 1, A + A + A: 2, B + A + C: 1, A + A + A + A: 1}
WORDS = {5: b"a", 300: b"bee", 20000: b"sea", 2: b"{?}", 3: b"{*}", 4: b"{**}"}
EDGES = [63, 64, 65, 255, 256, 257, 1023, 1024, 1025]


@pytest.mark.parametrize("n", EDGES)
def test_positions_in_a_line_at_the_block_and_scan_widths(ctx, n):
    """one line of n tokens, every position a hit at every length (lengths 1-4 of the same token): n, n - 1, n - 2, n - 3 hits in its runs"""
    rows = check(ctx, TINY, [[A] * n], words=WORDS)
    assert len(rows) == 4 * n - 6
    check(ctx, TINY, [[A] * n, [B], [A] * (n + 1)], minlength=2, maxlength=3, words=WORDS)


@pytest.mark.parametrize("n", EDGES)
def test_lines_and_rows_at_the_block_and_scan_widths(ctx, n):
    rnd = random.Random(n)
    lines = [[A]] * n  # n lines, n rows twice over (the whole-line row and the unigram)
    assert len(check(ctx, TINY, lines, words=WORDS)) == 2 * n
    lines = [rnd.choice([[A], [B, A, C], [C], [], [A, A], [C, A, B, A, C, C]]) for _ in range(n)]
    check(ctx, TINY, lines, exact=[rnd.random() < 0.3 for _ in range(n)], words=WORDS)


def test_one_line_no_rows_and_empty_lines(ctx):
    assert check(ctx, TINY, [[C, C, C]], words=WORDS) == []
    assert ctx.query_text(WORDS, 10) == b""
    assert check(ctx, TINY, [[A]], words=WORDS) == [(0, 0, A), (0, 0, A)]
    assert check(ctx, TINY, [[]] * 1025, words=WORDS) == []
    assert len(check(ctx, TINY, [[]] * 1025 + [[A, B]] + [[]] * 3, exact=[True] * 1029, words=WORDS)) == 1029
    assert check(ctx, TINY, [], words=WORDS) == []
    assert check(ctx, {}, [[A], [B]], minlength=1, maxlength=4) == []
    assert check(ctx, TINY, [[A, A, A]], minlength=4, maxlength=100) == [(0, 0, A + A + A)]  # the whole-line row does not depend on the lengths


def test_a_line_of_65536_tokens_is_served_and_one_more_is_refused(ctx):
    from colibri_amd import capi
    rows = check(ctx, TINY, [[A] * 65536, [B]])
    assert len(rows) == 4 * 65536 - 6 + 2 and rows[65535] == (0, 65535, A)
    arrays = model_arrays(TINY)
    with pytest.raises(capi.ColibriError) as e:
        ctx.query(payload_of([[B], [A] * 65537]), arrays[0], arrays[1], arrays[2])
    assert e.value.code == -7 and "65536" in str(e.value)
    check(ctx, TINY, [[A, B]], words=WORDS)  # the same context serves the next call


@pytest.mark.parametrize("chunk", [256, 257])
def test_lines_that_end_at_and_straddle_a_chunk_boundary(ctx, monkeypatch, chunk):
    """positions: a line of 255 tokens and its delimiter end exactly at position 256; the next line straddles 256 x 2 and 257 x 2"""
    monkeypatch.setenv("COLIBRI_QUERY_CHUNK", str(chunk))
    lines = [[A] * 255, [A] * 300, [B, A, C], [A] * 600, [], [A, B]]
    check(ctx, TINY, lines, words=WORDS)
    assert ctx.query_info()[0] == -(-sum(len(l) + 1 for l in lines) // chunk)


# ---- chunks, windows, budget --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["hamlet.v2.is", "edge.i"])
def test_chunks_cut_the_positions_anywhere(ctx, monkeypatch, case):
    counts, refs, tokens, words = load_case(case)
    lines, exact = batch(open(case_files(case)[2], "rb").read(), classes_of(words))
    lines, exact = lines + sentences(read_payload("hamlet.v2"))[:60], exact + [False] * 60
    npos = sum(len(l) + 1 for l in lines)
    for chunk in (None, 257, 64, 1):
        if chunk:
            monkeypatch.setenv("COLIBRI_QUERY_CHUNK", str(chunk))
        check(ctx, counts, lines, exact=exact, refs=refs)
        chunks, _, _, scratch = ctx.query_info()
        assert chunks == (-(-npos // chunk) if chunk else 1) and scratch > 0, chunk


@pytest.mark.parametrize("case", ["hamlet.v2.is", "edge.i"])
def test_windows_cut_prefixes_floats_references_and_words_anywhere(ctx, monkeypatch, case):
    counts, refs, tokens, words = load_case(case)
    lines, exact = batch(open(case_files(case)[2], "rb").read(), classes_of(words))
    arrays = model_arrays(counts, refs)
    rows = check(ctx, counts, lines, exact=exact, refs=refs)
    want = query_text(rows, lines, exact, counts, arrays, words, tokens)
    assert b"NOT FOUND" in want and b":0\t" in want
    for window in (None, 4096, 7, 1):
        if window:
            monkeypatch.setenv("COLIBRI_QUERY_WINDOW_BYTES", str(window))
        assert ctx.query_text(words, tokens) == want, window
        _, w, staging, _ = ctx.query_info()
        B_ = min(window or (64 << 20), len(want))
        assert w == -(-len(want) // B_) and staging == 2 * B_ and ctx.query_bytes == len(want)


@pytest.mark.parametrize("bits", [1, 3])
def test_hash_collisions_leave_identity_to_the_bytes(ctx, monkeypatch, bits):
    """the key table's hash cut to a few bits (insert and probe alike): every probe sequence is shared by many keys, the byte check decides"""
    monkeypatch.setenv("COLIBRI_QUERY_HASH_BITS", str(bits))
    counts, refs, tokens, words = load_case("hamlet.v2.is")
    lines, exact = batch(open(case_files("hamlet.v2.is")[2], "rb").read(), classes_of(words))
    check(ctx, counts, lines + sentences(read_payload("hamlet.v2")), exact=exact + [False] * 40, refs=refs, words=words, tokens=tokens)
    check(ctx, TINY, [[A] * 300, [B, A, C], [A, B], [C]], exact=[False, True, True, True], words=WORDS)


def test_refusals_leave_the_context_usable(ctx, monkeypatch):
    from colibri_amd import capi
    arrays = model_arrays(TINY)
    monkeypatch.setenv("COLIBRI_QUERY_BUDGET", "1000")
    with pytest.raises(capi.ColibriError) as e:
        ctx.query(payload_of([[A, B]] * 50), arrays[0], arrays[1], arrays[2])
    assert e.value.code == -7 and " need " in str(e.value)
    fixed = int(str(e.value).split(" need ")[1].split(" bytes")[0])  # what the call needs beside its chunk of positions
    with pytest.raises(capi.ColibriError) as e:
        ctx.query_text(WORDS, 10)  # (no result stands after a refusal)
    assert e.value.code == -6
    # a budget that holds everything but one chunk: 16 bytes x 4 lengths + 4 per position, for two positions at least
    monkeypatch.setenv("COLIBRI_QUERY_BUDGET", str(fixed + 8))
    with pytest.raises(capi.ColibriError) as e:
        ctx.query(payload_of([[A, B]] * 50), arrays[0], arrays[1], arrays[2])
    assert e.value.code == -7 and "per position" in str(e.value)
    # a budget that holds a chunk of one position, but no row beside it
    monkeypatch.setenv("COLIBRI_QUERY_CHUNK", "1")
    monkeypatch.setenv("COLIBRI_QUERY_BUDGET", str(fixed + 2 * 68))
    with pytest.raises(capi.ColibriError) as e:
        ctx.query(payload_of([[A, B]] * 50), arrays[0], arrays[1], arrays[2])
    assert e.value.code == -7 and "rows beside" in str(e.value)
    monkeypatch.delenv("COLIBRI_QUERY_CHUNK")
    monkeypatch.delenv("COLIBRI_QUERY_BUDGET")
    rows = check(ctx, TINY, [[A, B]] * 50, words=WORDS)
    # the text's own refusals: its bookkeeping per pattern and row, then two windows beside it; the rows stand, and the text comes once the budget does
    for budget, what in ((100, "patterns and"), (12 * 8 + 24 * (len(rows) + 1) + 64 + 2000, "exceed the budget")):
        monkeypatch.setenv("COLIBRI_QUERY_BUDGET", str(budget))
        with pytest.raises(capi.ColibriError) as e:
            ctx.query_text(WORDS, 10)
        assert e.value.code == -7 and "query text" in str(e.value) and what in str(e.value), budget
    monkeypatch.delenv("COLIBRI_QUERY_BUDGET")
    assert ctx.query_text(WORDS, 1000) == query_text(rows, [[A, B]] * 50, [False] * 50, TINY, arrays, WORDS, 1000)
    ctx.query(payload_of([[A]]), arrays[0], arrays[1])  # keys alone: rows, but no text
    with pytest.raises(capi.ColibriError) as e:
        ctx.query_text(WORDS, 10)
    assert e.value.code == -6


def test_flexgrams_and_gap_markers_are_tokens_like_any_other(ctx):
    flex, skip = varint(4), varint(3)
    counts = {A + flex + B: 2, A + skip + B: 1, A: 1}
    rows = check(ctx, counts, [[A, flex, B], [A, skip, B], [A, C, B], [A, A, B]], words=WORDS)
    assert (0, 0, A + flex + B) in rows and (1, 0, A + skip + B) in rows and all(k == A for s, _, k in rows if s >= 2)


# ---- the CLI --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_cli_device_route_equals_the_goldens(case):
    model, cls, lines = case_files(case)
    un = ["-u"] if case in ("hamlet.u", "hamlet.m2") else []
    out, err = cli(["-i", model, "-c", cls, "--queryfile", lines] + un, COLIBRI_QUERY="device")
    assert out == open(os.path.join(QUERY, case + ".Q.txt"), "rb").read() and "(query on the device: uploaded model)" in err
    args = ["-i", model, "-c", cls] + un
    for p in q_patterns(open(lines, "rb").read()):
        args += ["-q", p.decode()]
    out, err = cli(args, COLIBRI_QUERY="device")
    assert out == open(os.path.join(QUERY, case + ".q.txt"), "rb").read() and "(query on the device: uploaded model)" in err
