"""Pattern relations (colibri-patternmodeller --subsumes / --subsumed / --leftneighbours / --rightneighbours; IndexedPatternModel::getsubchildren /
getsubparents / getleftneighbours / getrightneighbours).

CPU part: a restatement of the reference's four functions (include/patternmodel.h:3166-3352 over getreverseindex :1746-1824), its skipgram
branches included, checked against the real reference's per-pattern results (tests/golden/relations/, see the README there) and against
hand-worked answers; the C++ face's host methods on the same models, with category / size / cutoff; the CLI's refusals that need no device;
the C ABI symbols. The GPU part (tests/test_gpu_relations.py) holds the device against this restatement."""
import gzip
import os
import subprocess

import pytest

from conftest import GOLDEN
from test_cooc import CLI, COOC, MODELS, SELFTEST, key_tokens, load_model, reverse_index, sentences
from test_oracle import read_payload

RELATIONS = os.path.join(GOLDEN, "relations")
FUNCTIONS = ("getsubchildren", "getsubparents", "getleftneighbours", "getrightneighbours")
KINDS = {f: k for k, f in enumerate(FUNCTIONS)}  # colibri_relations' kinds, in the header's order
THRESHOLDS = (0, 2)
GAP = b"\x03"


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def same_pattern(a, at, b, window):
    """PatternPointer::operator== (src/pattern.cpp:1067-1103) of A (the model's key, gaps as 03) and B (the corpus window under B's mask):
    equal byte lengths, equal masks, equal non-gap tokens. The gapped tokens of the window keep their own bytes, so a multi-byte token in
    a gap makes B differ from A even when both are the same skipgram"""
    return b == a and (GAP not in at or all(len(window[k]) == 1 for k, x in enumerate(at) if x == GAP))


def related(fn, a, at, t, i, b, window, toks):
    """does the occurrence of B at token i of the sentence (tokens toks) count for the occurrence of A at token t (reference lines in the
    header of each branch)"""
    na, n = len(at), len(window)
    bt = key_tokens(b)
    askip, bskip = GAP in at, GAP in bt
    if fn == "getrightneighbours":  # :3321-3352
        return i == t + na
    if fn == "getleftneighbours":  # :3278-3312
        return i + n == t
    if fn == "getsubchildren":  # :3166-3215
        if not (t <= i < t + na and n <= na - (i - t)) or same_pattern(a, at, b, window):
            return False
        if not askip and not bskip:
            return True
        # Pattern(pattern, i, n(B)) slices A at the corpus token index i (src/pattern.cpp:911-970): for an n-gram A past its end that is
        # all of A, which a skipgram B is never an instance of; for a skipgram A past its end it is empty. instanceof (:1764-1784) then
        # needs n(B) tokens, each equal to the slice's or under one of its gaps; an n-gram slice needs B to be the same n-gram.
        if not askip or i + n > na:
            return False
        sl = at[i:i + n]
        return all(x == GAP or toks[i + k] == x for k, x in enumerate(sl)) and (GAP in sl or not bskip)
    if fn == "getsubparents":  # :3222-3270
        if not (i <= t and n >= na + (t - i)) or same_pattern(a, at, b, window):
            return False
        if not askip and not bskip:
            return True
        # pattern.instanceof(candidate) (:3255): the tokens of a PatternPointer slice of B are corpus tokens, never a gap, so A must be an
        # n-gram with B's length (so B starts at t) and A's tokens, which it has where A occurs
        return not askip and n == na
    raise ValueError(fn)


def relations(fn, counts, refs, payload, threshold=0, category=0, size=0, rule=None):
    """fn(A, threshold, category, size) for every pattern A: {(A, B): count}. category 1 = n-grams, 2 = skipgrams (PatternCategory)"""
    rule = rule or related
    sents = sentences(payload)
    rev = reverse_index(counts, sents)
    out = {}
    for a, rl in refs.items():
        at = key_tokens(a)
        rel = {}
        for s, t in rl:
            toks = sents[s - 1]
            for i, n, b in rev[s - 1]:
                if threshold and counts[b] < threshold:
                    continue
                if category and (2 if GAP in key_tokens(b) else 1) != category:
                    continue
                if size and n != size:
                    continue
                if rule(fn, a, at, t, i, b, toks[i:i + n], toks):
                    rel[b] = rel.get(b, 0) + 1
        for b, c in rel.items():
            if threshold == 0 or c >= threshold:
                out[(a, b)] = c
    return out


def order_rows(rows):
    """the documented order: A's pattern number, then count descending, then B's key bytes"""
    return sorted(rows.items(), key=lambda kv: (kv[0][0], -kv[1], kv[0][1]))


# ---- fixtures -----------------------------------------------------------------------------------------------------------------------
def load_fixture(fn, corpus, kind, thr):
    out = {}
    for ln in gzip.open(os.path.join(RELATIONS, f"{fn}.{corpus}.{kind}.t{thr}.txt.gz"), "rt").read().splitlines():
        a, b, c = ln.split("\t")
        out[(bytes.fromhex(a), bytes.fromhex(b))] = int(c)
    return out


def read_rows(path):
    got = {}
    for ln in open(path).read().splitlines():
        a, b, c = ln.split("\t")
        got[(bytes.fromhex(a), bytes.fromhex(b))] = int(c)
    return got


@pytest.mark.parametrize("thr", THRESHOLDS)
@pytest.mark.parametrize("fn", FUNCTIONS)
@pytest.mark.parametrize("corpus,kind", MODELS)
def test_restatement_matches_the_reference(corpus, kind, fn, thr):
    counts, refs = load_model(corpus, kind)
    assert relations(fn, counts, refs, read_payload(corpus), thr) == load_fixture(fn, corpus, kind, thr)


def test_fixtures_exercise_the_skipgram_branches():
    """the reference's own skipgram tests decide rows in these fixtures: slicing A at the token offset i - t instead of the corpus index i would
    give other tables"""
    def by_offset(fn, a, at, t, i, b, window, toks):
        if fn == "getsubchildren" and GAP in at and t <= i:
            return related(fn, a, at, 0, i - t, b, window, toks[t:])
        return related(fn, a, at, t, i, b, window, toks)

    differs = [c for c in ("hamlet.v2", "zipf20k", "phrases15k", "edge")
               if relations("getsubchildren", *load_model(c, "is"), read_payload(c), rule=by_offset) != load_fixture("getsubchildren", c, "is", 0)]
    assert differs


# ---- hand-worked answers ------------------------------------------------------------------------------------------------------------
A, B, C, D = b"\x06", b"\x07", b"\x08", b"\x09"


def test_neighbours_count_the_pattern_itself_and_stop_at_sentence_ends():
    counts = {A: 3, B: 1}
    payload = A + A + B + b"\x00" + A + b"\x00"
    refs = {A: [(1, 0), (1, 1), (2, 0)], B: [(1, 2)]}
    assert relations("getrightneighbours", counts, refs, payload) == {(A, A): 1, (A, B): 1}
    assert relations("getleftneighbours", counts, refs, payload) == {(A, A): 1, (B, A): 1}


def test_subsumption_of_ngrams():
    AB, ABC, BC = A + B, A + B + C, B + C
    counts = {A: 1, B: 1, C: 1, AB: 1, BC: 1, ABC: 1}
    payload = A + B + C + b"\x00"
    refs = {A: [(1, 0)], B: [(1, 1)], C: [(1, 2)], AB: [(1, 0)], BC: [(1, 1)], ABC: [(1, 0)]}
    kids = relations("getsubchildren", counts, refs, payload)
    assert {b for (a, b) in kids if a == ABC} == {A, B, C, AB, BC}
    assert {b for (a, b) in kids if a == AB} == {A, B}
    parents = relations("getsubparents", counts, refs, payload)
    assert {b for (a, b) in parents if a == B} == {AB, BC, ABC}
    assert {b for (a, b) in parents if a == C} == {BC, ABC}


def test_skipgram_subchildren_slice_at_the_corpus_index():
    """A = A {*} C at token 2 of its sentence: the reference slices A at the corpus indices 2, 3, 4 — past A's three tokens from index 3 on — so
    only the slice at index 2 (A's last token, C) can hold a child; at token 0 the slices are A's own tokens"""
    S = A + b"\x03" + C
    counts = {S: 2, A: 2, C: 2}
    payload = A + B + C + b"\x00" + D + D + A + B + C + b"\x00"
    refs = {S: [(1, 0), (2, 2)], A: [(1, 0), (2, 2)], C: [(1, 2), (2, 4)]}
    got = relations("getsubchildren", counts, refs, payload)
    # occurrence (1, 0): A at 0 (slice [A]) and C at 2 (slice [C]); occurrence (2, 2): A at 2 against slice [C] fails, C at 4 is past A's end
    assert got == {(S, A): 1, (S, C): 1}


def test_skipgram_subparents_only_for_ngrams_under_a_skipgram_of_their_length():
    S, ABC = A + b"\x03" + C, A + B + C
    counts = {S: 1, ABC: 1, A: 1}
    payload = A + B + C + b"\x00"
    refs = {S: [(1, 0)], ABC: [(1, 0)], A: [(1, 0)]}
    got = relations("getsubparents", counts, refs, payload)
    assert got == {(ABC, S): 1, (A, ABC): 1}  # no parents of the skipgram; A's skipgram parent would need its length


def test_a_multibyte_token_under_a_gap_makes_a_skipgram_its_own_relation():
    W = b"\x85\x06"  # a two-byte token
    S = A + b"\x03" + C
    counts = {S: 2}
    payload = A + B + C + b"\x00" + A + W + C + b"\x00"
    refs = {S: [(1, 0), (2, 0)]}
    assert relations("getsubchildren", counts, refs, payload) == {(S, S): 1}  # found at (2, 0) under its multi-byte gap, B != A there


def test_order_rows_is_pattern_then_count_then_key():
    rows = {(B, A): 2, (A, B): 2, (A, A): 1, (A, C): 2}
    assert [k for k, _ in order_rows(rows)] == [(A, B), (A, C), (A, A), (B, A)]


# ---- the C++ face's host methods ----------------------------------------------------------------------------------------------------
def host_rows(tmp_path, corpus, kind, fn, thr, extra=()):
    out = str(tmp_path / "rel.txt")
    p = subprocess.run([SELFTEST, "relations_host", os.path.join(COOC, f"{corpus}.{kind}.colibri.patternmodel"), os.path.join(GOLDEN, corpus + ".colibri.dat"), fn, str(thr)]
                       + [str(x) for x in extra] + [out], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.strip() == "OK", p.stdout + p.stderr
    return read_rows(out)


@pytest.mark.parametrize("thr", THRESHOLDS)
@pytest.mark.parametrize("fn", FUNCTIONS)
@pytest.mark.parametrize("corpus,kind", MODELS)
def test_cxx_face_host_methods_match_the_reference(tmp_path, corpus, kind, fn, thr):
    assert host_rows(tmp_path, corpus, kind, fn, thr) == load_fixture(fn, corpus, kind, thr)


def relations_cut(fn, counts, refs, payload, threshold, category, size, cutoff):
    """the neighbours with a cutoff: distinct patterns in the order the scan meets them (the forward index, then position, length, the n-gram
    before its skipgrams, masks ascending: what the C++ face documents), the count frozen once `cutoff` patterns are in"""
    sents = sentences(payload)
    rev = reverse_index(counts, sents)
    out = {}
    for a, rl in refs.items():
        at = key_tokens(a)
        rel = {}
        for s, t in rl:
            toks = sents[s - 1]
            for i, n, b in rev[s - 1]:
                if (threshold and counts[b] < threshold) or (category and (2 if GAP in key_tokens(b) else 1) != category) or (size and n != size):
                    continue
                if related(fn, a, at, t, i, b, toks[i:i + n], toks):
                    rel[b] = rel.get(b, 0) + 1
                    if len(rel) >= cutoff:
                        break
            if len(rel) >= cutoff:
                break
        out.update({(a, b): c for b, c in rel.items() if threshold == 0 or c >= threshold})
    return out


@pytest.mark.parametrize("fn", FUNCTIONS)
@pytest.mark.parametrize("corpus", ["hamlet.v2", "edge"])
def test_cxx_face_category_size_cutoff(tmp_path, corpus, fn):
    counts, refs = load_model(corpus, "is")
    payload = read_payload(corpus)
    for thr, cat, size in ((0, 1, 0), (0, 2, 0), (2, 0, 3), (0, 2, 3), (2, 1, 2)):
        want = relations(fn, counts, refs, payload, thr, cat, size)
        assert host_rows(tmp_path, corpus, "is", fn, thr, (cat, size, 0)) == want
    assert relations(fn, counts, refs, payload, 0, 2, 0)  # (the skipgram-only tables are not empty)
    if "neighbours" in fn:
        for cut in (1, 3):
            want = relations_cut(fn, counts, refs, payload, 0, 0, 0, cut)
            assert host_rows(tmp_path, corpus, "is", fn, 0, (0, 0, cut)) == want
            assert want != relations(fn, counts, refs, payload)


# ---- CLI that needs no device -------------------------------------------------------------------------------------------------------
FLAGS = ("--subsumes", "--subsumed", "--leftneighbours", "--rightneighbours")


def test_cli_relation_flags_need_a_class_file():
    for flag in FLAGS:
        out = subprocess.run([CLI, "-i", os.path.join(COOC, "hamlet.v2.i.colibri.patternmodel"), "-f", os.path.join(GOLDEN, "hamlet.v2.colibri.dat"), flag],
                             capture_output=True, text=True)
        assert out.returncode == 2 and f"{flag} needs a class file" in out.stderr, out.stderr


def test_cli_relation_flags_need_a_reverse_index():
    for flag in FLAGS:
        out = subprocess.run([CLI, "-i", os.path.join(COOC, "hamlet.v2.i.colibri.patternmodel"), "-c", os.path.join(GOLDEN, "hamlet.colibri.cls"), flag],
                             capture_output=True, text=True)
        assert out.returncode != 0 and "No reverse index present" in out.stderr, out.stderr


def test_cli_unindexed_model_prints_the_patterns_only():
    """--subsumes on an unindexed model: every pattern, no header, no relation (the base class's outputrelations, reference :2628)"""
    model = os.path.join(GOLDEN, "hamlet.v1.colibri.patternmodel")
    for flag in FLAGS:
        out = subprocess.run([CLI, "-i", model, "-u", "-c", os.path.join(GOLDEN, "hamlet.colibri.cls"), flag], capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        lines = out.stdout.splitlines()
        assert len(lines) == 111 and not any("\t" in ln for ln in lines)


def test_cli_still_refuses_g_and_the_cooc_relations():
    for flag in (["-g"], ["--leftcooc"], ["--rightcooc"]):
        out = subprocess.run([CLI, "-f", os.path.join(GOLDEN, "hamlet.v2.colibri.dat")] + flag, capture_output=True, text=True)
        assert out.returncode == 2, out.stderr


def test_abi_declares_the_relation_entry_points():
    import sys
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "colibri-core_amd", "pyhost"))
    from colibri_amd import capi
    hdr = open(os.path.join(ROOT, "include", "colibri_hip.h")).read()
    for name in ("colibri_relations", "colibri_relations_resident", "colibri_relations_fetch", "colibri_relations_info"):
        assert name + "(" in hdr and name in capi.EXPORTED
    for name, k in (("COLIBRI_REL_SUBCHILDREN", 0), ("COLIBRI_REL_SUBPARENTS", 1), ("COLIBRI_REL_LEFTNEIGHBOURS", 2), ("COLIBRI_REL_RIGHTNEIGHBOURS", 3)):
        assert f"{name} = {k}" in hdr
        assert KINDS[FUNCTIONS[k]] == k
    assert (capi.REL_SUBCHILDREN, capi.REL_SUBPARENTS, capi.REL_LEFTNEIGHBOURS, capi.REL_RIGHTNEIGHBOURS) == (0, 1, 2, 3)
    assert "#define COLIBRI_ABI_VERSION 4 " in hdr
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "colibri-core_amd", "lib", "libcolibri_hip.so")], capture_output=True, text=True).stdout
    for name in ("colibri_relations", "colibri_relations_resident", "colibri_relations_fetch", "colibri_relations_info"):
        assert f" T {name}\n" in nm
