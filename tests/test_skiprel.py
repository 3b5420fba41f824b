"""The three relations of skipgrams (IndexedPatternModel::getskipcontent / getinstances / gettemplates; colibri-patternmodeller --skipcontent).

CPU part: a restatement of the three functions as the C++ face's host methods state them (reference include/patternmodel.h:3029-3157), checked
against the real reference's per-pattern results (tests/golden/skiprel/, see the README there), against the reference's own text output
(tests/golden/relations.<corpus>.<tag>.*.txt) and against hand-worked answers; the host methods on the same models; the C ABI's declarations.
The GPU part (tests/test_gpu_skiprel.py) holds the device against the fixtures and this restatement."""
import gzip
import os
import struct
import subprocess
import sys

import pytest

from conftest import GOLDEN, ROOT
from test_compare import decode, read_classes
from test_cooc import SELFTEST, key_tokens, sentences
from test_oracle import read_payload

sys.path.insert(0, os.path.join(ROOT, "oracle"))
import oracle  # noqa: E402

SKIPREL = os.path.join(GOLDEN, "skiprel")
MODELS = [(c, t) for c in ("hamlet.v2", "zipf20k", "phrases15k") for t in ("is", "isT1")]  # the reference's -s -l 5 -t 2 -T 2|1 models
FUNCTIONS = ("getinstances", "gettemplates", "getskipcontent")
THRESHOLDS = (0, 3)
GAP = b"\x03"
_cache = {}


def load_model(corpus, tag):
    """(counts, refs, tokens, types) of the golden dump <corpus>.<tag>.l5.txt, read once"""
    if (corpus, tag) not in _cache:
        m = oracle.parse_dump(open(os.path.join(GOLDEN, f"{corpus}.{tag}.l5.txt")).read(), indexed=True)
        _cache[(corpus, tag)] = (m.counts, m.refs, m.tokens, m.types)
    return _cache[(corpus, tag)]


def load_fixture(fn, corpus, tag, thr=0):
    name = f"{fn}.{corpus}.{tag}" + ("" if fn == "getskipcontent" else f".t{thr}") + ".txt.gz"
    out = {}
    for ln in gzip.open(os.path.join(SKIPREL, name), "rt").read().splitlines():
        a, b, c = ln.split("\t")
        out[(bytes.fromhex(a), bytes.fromhex(b))] = int(c)
    return out


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def masked_pointer_equals(data, mask, other):
    """PatternPointer::operator==(const Pattern&) for the window bytes `data` under `mask` against the key `other` (src/pattern.cpp:1009-1041):
    byte by byte AT THE SAME INDEX; a byte past `other` reads as 0"""
    def at(i):
        return other[i] if i < len(other) else 0
    if not data or data[0] == 0:
        return len(other) == 0
    if not other:
        return False
    tok = 0
    for i, d in enumerate(data):
        if i > 0 and at(i - 1) >= 128 and at(i) == 0:
            return False
        if mask and d < 128:
            if tok <= 30 and (mask >> tok) & 1:
                if at(i) != 3:
                    return False
            elif d != at(i):
                return False
            tok += 1
        elif d != at(i):
            return False
    return at(len(data)) == 0


def gap_masks(counts):
    out = {}
    for k in counts:
        t = key_tokens(k)
        if GAP in t:
            out.setdefault(len(t), set()).add(sum(1 << i for i, x in enumerate(t) if x == GAP))
    return {n: sorted(v) for n, v in out.items()}


def skiprel(fn, counts, refs, payload, thr=0):
    """fn(A, thr) for every pattern A: {(A, B or content): count}. A reference whose window leaves its sentence is skipped"""
    sents = sentences(payload)
    masks = gap_masks(counts)
    out = {}
    for a in refs:
        at = key_tokens(a)
        n = len(at)
        gaps = [i for i, x in enumerate(at) if x == GAP]
        rel = {}
        if fn == "getskipcontent" and not gaps:
            continue
        if fn == "gettemplates" and (n < 3 or not masks or (thr and counts[a] < thr)):
            continue
        for s, t in refs[a]:
            toks = sents[s - 1] if 0 < s <= len(sents) else []
            if t + n > len(toks):
                continue
            w = toks[t:t + n]
            if fn == "getskipcontent":
                b = b"".join(w[gaps[0]:gaps[-1] + 1])
                rel[b] = rel.get(b, 0) + 1
            elif fn == "getinstances":
                b = b"".join(w)
                if b != a and b in counts and (thr == 0 or counts[b] >= thr):
                    rel[b] = rel.get(b, 0) + 1
            else:
                for m in masks.get(n, ()):
                    b = b"".join(GAP if (m >> j) & 1 else w[j] for j in range(n))
                    if b in counts and not masked_pointer_equals(b"".join(w), m, a):
                        rel[b] = rel.get(b, 0) + 1
        out.update({(a, b): c for b, c in rel.items() if fn == "getskipcontent" or thr == 0 or c >= thr})
    return out


@pytest.mark.parametrize("fn", FUNCTIONS)
@pytest.mark.parametrize("corpus,tag", MODELS)
def test_restatement_matches_the_reference(corpus, tag, fn):
    counts, refs, _, _ = load_model(corpus, tag)
    payload = read_payload(corpus)
    for thr in THRESHOLDS if fn != "getskipcontent" else (0,):
        assert skiprel(fn, counts, refs, payload, thr) == load_fixture(fn, corpus, tag, thr), thr


def test_fixtures_exercise_what_they_are_for():
    """self-template rows are there, the threshold drops rows but not all, a content has up to 6 bytes, as many instance rows as skip-content rows"""
    for (corpus, tag), (sk_rows, tmpl, selfs) in {("hamlet.v2", "is"): (28, 56, 0), ("hamlet.v2", "isT1"): (113, 535, 0), ("zipf20k", "is"): (748, 887, 11),
                                                     ("phrases15k", "is"): (695, 855, 99), ("phrases15k", "isT1"): (4840, 21637, None)}.items():
        counts = load_model(corpus, tag)[0]
        sk, ins, tm = load_fixture("getskipcontent", corpus, tag), load_fixture("getinstances", corpus, tag), load_fixture("gettemplates", corpus, tag)
        assert len(sk) == sk_rows and len(ins) == sk_rows and len(tm) == tmpl
        assert all(b in counts for _, b in sk)  # every content is in the model
        if selfs is not None:
            assert sum(1 for a, b in tm if a == b) == selfs
    for corpus, left, of in (("zipf20k", 294, 748), ("phrases15k", 196, 695)):
        t0, t3 = load_fixture("getinstances", corpus, "is", 0), load_fixture("getinstances", corpus, "is", 3)
        assert len(t3) == left and len(t0) == of and set(t3.items()) < set(t0.items())
        m0, m3 = load_fixture("gettemplates", corpus, "is", 0), load_fixture("gettemplates", corpus, "is", 3)
        assert 0 < len(m3) < len(m0) and set(m3.items()) < set(m0.items())
    assert max(len(b) for _, b in load_fixture("getskipcontent", "phrases15k", "isT1")) == 6
    assert max(len(key_tokens(b)) for _, b in load_fixture("getskipcontent", "phrases15k", "isT1")) >= 2


TEXT = [("hamlet.v2", "isT1"), ("hamlet.v2", "is"), ("phrases15k", "is"), ("zipf20k", "is")]


@pytest.mark.parametrize("fn,flt,label", [("getskipcontent", "skipcontent", "INSTANTIATED-BY"), ("getinstances", "instances_api", "INSTANCE-OF"),
                                          ("gettemplates", "templates_api", "TEMPLATE-OF")])
@pytest.mark.parametrize("corpus,tag", TEXT)
def test_fixtures_are_the_references_printed_rows(corpus, tag, fn, flt, label):
    """the fixtures at threshold 0, decoded through the class file, are the relation lines of the reference's own text output"""
    cls = read_classes(os.path.join(GOLDEN, "hamlet.colibri.cls" if corpus.startswith("hamlet") else "synthetic.colibri.cls"))
    counts = load_model(corpus, tag)[0]
    rows = load_fixture(fn, corpus, tag, 0)
    total = {}
    for (a, _), c in rows.items():
        total[a] = total.get(a, 0) + c
    mine = sorted(f"\t{decode(a, cls)}\t{label}\t{decode(b, cls)}\t{c}\t{c / total[a]:g}\t{counts.get(b, 0)}" for (a, b), c in rows.items())
    want = [ln for ln in open(os.path.join(GOLDEN, f"relations.{corpus}.{tag}.{flt}.txt")).read().splitlines() if ln.startswith("\t")]
    assert mine == sorted(want) and mine


# ---- hand-worked answers ------------------------------------------------------------------------------------------------------------
A, B, C, D = b"\x06", b"\x07", b"\x08", b"\x09"
W = b"\x85\x06"  # a two-byte token


def test_two_gaps_keep_the_token_between_them():
    S = A + GAP + C + GAP + D  # head 1, tail 1: the content is tokens 1..3
    counts = {S: 2, B + C + B: 1}
    payload = A + B + C + B + D + b"\x00" + A + D + C + A + D + b"\x00"
    refs = {S: [(1, 0), (2, 0)], B + C + B: [(1, 1)]}
    assert skiprel("getskipcontent", counts, refs, payload) == {(S, B + C + B): 1, (S, D + C + A): 1}


def test_a_multibyte_token_under_a_gap():
    S = A + GAP + C
    counts = {S: 3, A + B + C: 1}
    payload = A + B + C + b"\x00" + A + W + C + b"\x00" + A + W + C + b"\x00"
    refs = {S: [(1, 0), (2, 0), (3, 0)], A + B + C: [(1, 0)]}
    assert skiprel("getskipcontent", counts, refs, payload) == {(S, B): 1, (S, W): 2}  # a two-byte content
    # the window under S's own mask is S, but the byte-at-the-same-index comparison only sees that where the gapped token is one byte
    assert skiprel("gettemplates", counts, refs, payload) == {(S, S): 2, (A + B + C, S): 1}
    assert skiprel("gettemplates", counts, refs, payload, 2) == {(S, S): 2}  # A's own count, then the joint count
    assert skiprel("getinstances", counts, refs, payload) == {(S, A + B + C): 1}


def test_an_ngram_has_no_instances_and_no_content():
    counts = {A + B + C: 2, A + GAP + C: 2}
    payload = A + B + C + b"\x00" + A + B + C + b"\x00"
    refs = {A + B + C: [(1, 0), (2, 0)], A + GAP + C: [(1, 0), (2, 0)]}
    got = skiprel("getinstances", counts, refs, payload)
    assert got == {(A + GAP + C, A + B + C): 2}
    assert not [k for k in skiprel("getskipcontent", counts, refs, payload) if k[0] == A + B + C]


def test_a_window_that_leaves_its_sentence_is_skipped():
    S = A + GAP + C
    counts = {S: 3, A + B + C: 1}
    payload = A + B + C + b"\x00" + A + B + b"\x00" + C + b"\x00"
    refs = {S: [(1, 0), (2, 0), (2, 1)], A + B + C: [(1, 0)]}  # (2, 0) and (2, 1) run past sentence 2 (a loaded model may hold such references)
    assert skiprel("getskipcontent", counts, refs, payload) == {(S, B): 1}
    assert skiprel("getinstances", counts, refs, payload) == {(S, A + B + C): 1}
    assert skiprel("gettemplates", counts, refs, payload) == {(A + B + C, S): 1}


# ---- the C++ face's host methods ----------------------------------------------------------------------------------------------------
def write_model(path, counts, refs, tokens, types):
    """an indexed model file, version 2 (the layout test_host_face.parse_model reads)"""
    with open(path, "wb") as f:
        f.write(bytes([0, 20, 2]) + struct.pack("<QQQ", tokens, types, len(counts)))
        for k in counts:
            f.write(k + b"\x00" + struct.pack("<I", counts[k]))
            for s, t in refs[k]:
                f.write(struct.pack("<IH", s, t))


def selftest_rows(tmp_path, mode, corpus, tag, fn, thr):
    counts, refs, tokens, types = load_model(corpus, tag)
    model, out = str(tmp_path / "m.colibri.patternmodel"), str(tmp_path / "rows.txt")
    write_model(model, counts, refs, tokens, types)
    p = subprocess.run([SELFTEST, mode, model, os.path.join(GOLDEN, corpus + ".colibri.dat"), fn, str(thr), out], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.strip() == "OK", p.stdout + p.stderr
    got = {}
    for ln in open(out).read().splitlines():
        a, b, c = ln.split("\t")
        got[(bytes.fromhex(a), bytes.fromhex(b))] = int(c)
    return got


@pytest.mark.parametrize("fn", FUNCTIONS)
@pytest.mark.parametrize("corpus,tag", MODELS)
def test_cxx_face_host_methods_match_the_reference(tmp_path, corpus, tag, fn):
    for thr in THRESHOLDS if fn != "getskipcontent" else (0,):
        assert selftest_rows(tmp_path, "skiprel_host", corpus, tag, fn, thr) == load_fixture(fn, corpus, tag, thr), thr


def test_abi_declares_the_skipgram_relation_entry_points():
    sys.path.insert(0, os.path.join(ROOT, "colibri-core_amd", "pyhost"))
    from colibri_amd import capi
    hdr = open(os.path.join(ROOT, "include", "colibri_hip.h")).read()
    names = ("colibri_skipcontent", "colibri_skipcontent_resident", "colibri_skipcontent_fetch", "colibri_skipcontent_info")
    for name in names:
        assert name + "(" in hdr and name in capi.EXPORTED
    assert "COLIBRI_REL_INSTANCES = 4" in hdr and "COLIBRI_REL_TEMPLATES = 5" in hdr
    assert (capi.REL_INSTANCES, capi.REL_TEMPLATES) == (4, 5)
    assert "#define COLIBRI_ABI_VERSION 4 " in hdr
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "colibri-core_amd", "lib", "libcolibri_hip.so")], capture_output=True, text=True).stdout
    for name in names:
        assert f" T {name}\n" in nm
