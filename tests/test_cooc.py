"""Sentence co-occurrence (colibri-patternmodeller -C / -Y; IndexedPatternModel::getcooc / outputcooc / outputcooc_npmi).

CPU part: a small restatement of the reference's getcooc (include/patternmodel.h:3542-3576 over getreverseindex_bysentence :1746-1862)
and npmi (:3582-3587), checked against the real reference's per-pattern getcooc (tests/golden/cooc/, see the README there), against
hand-worked answers, and against the NPMI formula's integer types (the counts' product is a size_t and does not wrap, the total is an
unsigned int); the C++ face's host getcooc on the same models; the CLI's refusals that need no device; the C ABI symbols. The GPU part (tests/test_gpu_cooc.py) holds the device against this restatement."""
import gzip
import math
import os
import subprocess

import pytest

from conftest import GOLDEN, ROOT
from test_host_face import parse_model
from test_oracle import read_payload

COOC = os.path.join(GOLDEN, "cooc")
BIN = os.path.join(ROOT, "colibri-core_amd", "bin")
SELFTEST = os.path.join(BIN, "host_selftest")
CLI = os.path.join(BIN, "colibri-patternmodeller")

# (corpus, model kind): the fixture models tests/golden/cooc/<corpus>.<kind>.colibri.patternmodel, trained by the reference
MODELS = [(c, k) for c in ("hamlet.v2", "zipf20k", "phrases15k", "edge") for k in ("i", "is")]
THRESHOLDS = (0, 1, 2, 3)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def key_tokens(key):
    out, start = [], 0
    for j, b in enumerate(key):
        if b < 128:
            out.append(key[start:j + 1])
            start = j + 1
    return out


def sentences(payload):
    """the corpus as token lists, sentence k (from 1) at index k - 1; every 00 ends one (empty sentences included)"""
    toks, start, out = [], 0, []
    for j, b in enumerate(payload):
        if b >= 128:
            continue
        tok = payload[start:j + 1]
        start = j + 1
        if tok == b"\x00":
            out.append(toks)
            toks = []
        else:
            toks.append(tok)
    if toks:
        out.append(toks)
    return out


def skipmasks(counts):
    """(length -> gap masks) of the skipgrams of the model: what matchskipgramhelper (:1722-1744) offers at a window"""
    out = {}
    for k in counts:
        t = key_tokens(k)
        if b"\x03" in t:
            m = sum(1 << i for i, x in enumerate(t) if x == b"\x03")
            out.setdefault(len(t), set()).add(m)
    return {n: sorted(v) for n, v in out.items()}


def reverse_index(counts, sents):
    """getreverseindex_bysentence for every sentence: [(token, n, key)] per sentence, found by looking the corpus' windows up in the model.
    A masked window is looked up by its materialised key (every gapped token becomes the byte 03), as the C++ face's gettemplates does."""
    lens = [len(key_tokens(k)) for k in counts]
    minn, maxn = (min(lens), max(lens)) if lens else (1, 0)
    masks = skipmasks(counts)
    out = []
    for toks in sents:
        occ = []
        for i in range(len(toks)):
            for n in range(minn, min(maxn, len(toks) - i) + 1):
                w = toks[i:i + n]
                key = b"".join(w)
                if key in counts:
                    occ.append((i, n, key))
                for m in masks.get(n, ()) if n >= 3 else ():
                    mk = b"".join(b"\x03" if (m >> j) & 1 else w[j] for j in range(n))
                    if mk in counts:
                        occ.append((i, n, mk))
        out.append(occ)
    return out


def cooc(counts, refs, payload, threshold=0):
    """sum over every pattern A of getcooc(A, threshold): {(A, B): joint count}. A's occurrences come from its forward index, B's from the corpus"""
    sents = sentences(payload)
    rev = reverse_index(counts, sents)
    out = {}
    for a, rl in refs.items():
        na = len(key_tokens(a))
        rel = {}
        for s, t in rl:
            for t2, n2, b in rev[s - 1]:
                if (t2 + n2 < t or t2 > t + na) and (threshold == 0 or counts[b] >= threshold):
                    rel[b] = rel.get(b, 0) + 1
        for b, c in rel.items():
            if threshold == 0 or c >= threshold:
                out[(a, b)] = c
    return out


def npmi(joint, ca, cb, total):
    """:3582-3587. occurrencecount returns size_t (:1653-1669), so the product of the two counts is 64-bit and does not wrap at 2^32; the group
    total is totaloccurrencesingroup(0, 0), an unsigned int (:2000-2004)"""
    return math.log(joint / (ca * cb)) / -math.log(joint / (total & 0xFFFFFFFF))


def npmi_rows(counts, table, x):
    total = sum(counts.values()) & 0xFFFFFFFF
    return {k: v for k, v in ((k, npmi(c, counts[k[0]], counts[k[1]], total)) for k, c in table.items()) if v >= x}


def order_rows(rows):
    """the documented order: value descending, then A's key bytes, then B's key bytes, ascending"""
    return sorted(rows.items(), key=lambda kv: (-kv[1], kv[0][0], kv[0][1]))


# ---- fixtures -----------------------------------------------------------------------------------------------------------------------
def load_model(corpus, kind):
    _, tokens, types, counts, refs = parse_model(os.path.join(COOC, f"{corpus}.{kind}.colibri.patternmodel"))
    return counts, refs


def load_fixture(corpus, kind, thr):
    path = os.path.join(COOC, f"getcooc.{corpus}.{kind}.t{0 if thr == 1 else thr}.txt.gz")  # t1 = t0 for these models (every count >= 1)
    out = {}
    for ln in gzip.open(path, "rt").read().splitlines():
        a, b, c = ln.split("\t")
        out[(bytes.fromhex(a), bytes.fromhex(b))] = int(c)
    return out


@pytest.mark.parametrize("thr", THRESHOLDS)
@pytest.mark.parametrize("corpus,kind", MODELS)
def test_restatement_matches_the_references_getcooc(corpus, kind, thr):
    counts, refs = load_model(corpus, kind)
    assert cooc(counts, refs, read_payload(corpus), thr) == load_fixture(corpus, kind, thr)


# ---- hand-worked answers ------------------------------------------------------------------------------------------------------------
A, B, C, D = b"\x06", b"\x07", b"\x08", b"\x09"


def test_adjacent_occurrences_do_not_count_a_gap_of_one_does():
    counts = {A: 2, B: 2}
    payload = A + B + b"\x00" + A + C + B + b"\x00"
    refs = {A: [(1, 0), (2, 0)], B: [(1, 1), (2, 2)]}
    got = cooc(counts, refs, payload)
    assert got == {(A, B): 1, (B, A): 1}


def test_self_pairs_and_repeated_occurrences():
    counts = {A: 3}
    payload = A + C + A + C + A + b"\x00"
    refs = {A: [(1, 0), (1, 2), (1, 4)]}
    # (0, 2), (0, 4), (2, 0), (2, 4), (4, 0), (4, 2): every ordered pair of distinct, non-adjacent occurrences
    assert cooc(counts, refs, payload) == {(A, A): 6}
    assert cooc(counts, refs, payload, threshold=3) == {(A, A): 6}
    assert cooc(counts, refs, payload, threshold=4) == {}  # B's own count (3) is below the threshold


def test_empty_sentences_and_sentence_boundaries():
    counts = {A: 2, B: 2}
    payload = A + b"\x00\x00" + C + B + b"\x00" + A + C + B + b"\x00"
    refs = {A: [(1, 0), (4, 0)], B: [(3, 1), (4, 2)]}
    assert cooc(counts, refs, payload) == {(A, B): 1, (B, A): 1}  # only sentence 4 holds both


def test_bigram_neighbours_need_a_gap_after_their_end():
    AB = A + B
    counts = {A: 1, AB: 1, D: 1}
    payload = A + B + C + D + b"\x00"
    refs = {A: [(1, 0)], AB: [(1, 0)], D: [(1, 3)]}
    got = cooc(counts, refs, payload)
    # D at 3 lies after A (3 > 0 + 1) and after AB (3 > 0 + 2); from D's side A (0 + 1 < 3) and AB (0 + 2 < 3) lie before it; A and AB overlap
    assert got == {(A, D): 1, (AB, D): 1, (D, A): 1, (D, AB): 1}


def test_skipgram_found_in_the_corpus_but_not_in_its_own_index():
    """B = A {*} C is looked up in the corpus at every window; its forward index holds only the occurrence its kept n-gram gave it"""
    S = A + b"\x03" + C
    counts = {S: 1, D: 2}
    payload = A + B + C + D + D + D + b"\x00" + D + D + A + D + C + b"\x00"
    refs = {S: [(1, 0)], D: [(1, 4), (2, 0)]}
    got = cooc(counts, refs, payload)
    # D at (1, 4): S at (1, 0) ends at 3 < 4 -> counts; D at (2, 0): S found in the corpus at (2, 2), 2 > 0 + 1 -> counts
    assert got[(D, S)] == 2
    # S's own side has one reference, (1, 0): D at 4 and 5 count (> 0 + 3), D at 3 is adjacent
    assert got[(S, D)] == 2


def test_npmi_product_does_not_wrap_the_total_does():
    """two counts of 70000: their product passes 2^32 and stays whole (size_t); a group total past 2^32 is taken modulo 2^32 (unsigned int)"""
    ca, cb, joint, total = 70000, 70000, 5, 10 ** 9
    assert ca * cb > 1 << 32
    assert npmi(joint, ca, cb, total) == math.log(5 / 4.9e9) / -math.log(5 / 1e9)
    assert npmi(joint, ca, cb, total) != math.log(joint / ((ca * cb) & 0xFFFFFFFF)) / -math.log(joint / total)
    assert npmi(joint, ca, cb, (1 << 32) + 10 ** 9) == npmi(joint, ca, cb, 10 ** 9)


def test_order_rows_is_value_then_keys():
    rows = {(B, A): 2, (A, B): 2, (A, A): 3, (A, C): 2}
    assert [k for k, _ in order_rows(rows)] == [(A, A), (A, B), (A, C), (B, A)]


# ---- the C++ face's host getcooc ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thr", THRESHOLDS)
@pytest.mark.parametrize("corpus,kind", MODELS)
def test_cxx_face_host_getcooc_matches_the_references(tmp_path, corpus, kind, thr):
    out = str(tmp_path / "cooc.txt")
    p = subprocess.run([SELFTEST, "getcooc", os.path.join(COOC, f"{corpus}.{kind}.colibri.patternmodel"), os.path.join(GOLDEN, corpus + ".colibri.dat"), str(thr), out],
                       capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.strip() == "OK", p.stdout + p.stderr
    got = {}
    for ln in open(out).read().splitlines():
        a, b, c = ln.split("\t")
        got[(bytes.fromhex(a), bytes.fromhex(b))] = int(c)
    assert got == load_fixture(corpus, kind, thr)


# ---- CLI refusals that need no device ----------------------------------------------------------------------------------------------
def test_cli_cooc_needs_a_class_file():
    for flag in (["-C", "2"], ["-Y", "0.1"]):
        out = subprocess.run([CLI, "-i", os.path.join(COOC, "hamlet.v2.i.colibri.patternmodel"), "-f", os.path.join(GOLDEN, "hamlet.v2.colibri.dat")] + flag,
                             capture_output=True, text=True)
        assert out.returncode == 2 and "needs a class file" in out.stderr, out.stderr


def test_cli_cooc_needs_a_corpus():
    out = subprocess.run([CLI, "-i", os.path.join(COOC, "hamlet.v2.i.colibri.patternmodel"), "-c", os.path.join(GOLDEN, "hamlet.colibri.cls"), "-C", "2"],
                         capture_output=True, text=True)
    assert out.returncode != 0 and "corpus" in out.stderr, out.stderr


def test_abi_declares_the_cooc_entry_points():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "colibri-core_amd", "pyhost"))
    from colibri_amd import capi
    hdr = open(os.path.join(ROOT, "include", "colibri_hip.h")).read()
    for name in ("colibri_cooc", "colibri_cooc_resident", "colibri_cooc_fetch"):
        assert name + "(" in hdr and name in capi.EXPORTED
    assert "#define COLIBRI_ABI_VERSION 4 " in hdr
