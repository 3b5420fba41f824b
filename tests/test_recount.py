"""The skipgrams of an in-place rebuild (colibri-patternmodeller -I -s; PatternModel::trainskipgrams_selfconstrained, reference
include/patternmodel.h:1569-1604; csrc/recount.hpp), without a device.

A plain restatement, recount(): a skipgram of n >= 3 tokens with gap mask m occurs at (s, t) iff t + n <= sentencelength(s) and every token
outside m equals the skipgram's. It is checked against what the reference's own colibri-patternmodeller -I -s prints for the fixture models
(tests/golden/recount/, see the README there); then the C++ face's host route (COLIBRI_RECOUNT=host, tests/recount_check.cpp) is held to the
restatement on all four corpora, the one with empty sentences included. tests/test_gpu_recount.py holds the device to the same restatement."""
import gzip
import os
import subprocess

import pytest

from conftest import GOLDEN, ROOT
from test_cooc import COOC, key_tokens, load_model, sentences, skipmasks
from test_coverage import tokens_of
from test_oracle import read_payload
from test_print import read_classes, text_of

RECOUNT = os.path.join(GOLDEN, "recount")
PKG = os.path.join(ROOT, "colibri-core_amd")
# corpus -> (class file, the thresholds of the fixtures: 2, and one under which the load drops skipgrams)
FIXTURES = {"hamlet.v2": ("hamlet.colibri.cls", (2, 5)), "zipf20k": ("synthetic.colibri.cls", (2, 50)), "phrases15k": ("synthetic.colibri.cls", (2, 60))}
CORPORA = ("hamlet.v2", "zipf20k", "phrases15k", "edge")


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def is_skipgram(key):
    return b"\x03" in key_tokens(key)


def recount_all(skipgram_keys, sents, first_sentence=1):
    """{key: [(sentence, token), ...]} for every key, in corpus order; sents: the corpus as token lists (test_cooc.sentences)"""
    keys = set(skipgram_keys)
    masks = skipmasks(keys)
    out = {k: [] for k in keys}
    for s, toks in enumerate(sents):
        for t in range(len(toks)):
            for n, ms in masks.items():
                if n < 3 or t + n > len(toks):
                    continue
                w = toks[t:t + n]
                for m in ms:
                    mk = b"".join(b"\x03" if (m >> j) & 1 else w[j] for j in range(n))
                    if mk in out:
                        out[mk].append((first_sentence + s, t))
    return out


def recount(skipgram_keys, sents, mintokens, first_sentence=1):
    """what trainskipgrams_selfconstrained leaves of the skipgrams: those found mintokens times or more, with their references"""
    return {k: v for k, v in recount_all(skipgram_keys, sents, first_sentence).items() if len(v) >= mintokens}


def loaded_skipgrams(corpus, mintokens):
    """the skipgrams of the fixture model that a load under the threshold keeps (the stored count decides)"""
    counts, _ = load_model(corpus, "is")
    return [k for k, c in counts.items() if is_skipgram(k) and c >= mintokens]


_SENTS = {}


def corpus_sentences(corpus):
    if corpus not in _SENTS:
        _SENTS[corpus] = sentences(read_payload(corpus))
    return _SENTS[corpus]


def skipgram_rows(text):
    """the skipgram rows of a -P text as a sorted list of (pattern text, count, references text | None)"""
    rows = []
    for line in text.split(b"\n"):
        col = line.split(b"\t")
        if len(col) >= 7 and col[4] == b"skipgram":
            rows.append((col[0], int(col[1]), col[7].strip() if len(col) > 7 else None))
    return sorted(rows)


def restated_rows(found, words, indexed):
    return sorted((text_of(tokens_of(k), words), len(v), b" ".join(b"%d:%d" % r for r in v) if indexed else None) for k, v in found.items())


def fixture_text(corpus, kind, thr):
    return gzip.open(os.path.join(RECOUNT, f"rebuild.{corpus}.{kind}.t{thr}.txt.gz"), "rb").read()


# ---- the restatement against the reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("corpus", sorted(FIXTURES))
@pytest.mark.parametrize("kind", ["i", "u"])
def test_restatement_equals_the_reference(corpus, kind):
    cls, thresholds = FIXTURES[corpus]
    words = read_classes(os.path.join(GOLDEN, cls))
    kept = []
    for thr in thresholds:
        want = skipgram_rows(fixture_text(corpus, kind, thr))
        got = restated_rows(recount(loaded_skipgrams(corpus, thr), corpus_sentences(corpus), thr), words, kind == "i")
        assert got == want, (corpus, kind, thr)
        kept.append(len(want))
    assert kept[0] > 0 and kept[1] < kept[0]  # the second threshold drops skipgrams


def test_restatement_on_the_issue_example():
    """To {*} or: stored with count 4, found six times"""
    counts, _ = load_model("hamlet.v2", "is")
    words = read_classes(os.path.join(GOLDEN, "hamlet.colibri.cls"))
    rows = {r[0]: r for r in restated_rows(recount(loaded_skipgrams("hamlet.v2", 2), corpus_sentences("hamlet.v2"), 2), words, True)}
    assert rows[b"To {*} or"] == (b"To {*} or", 6, b"1:0 36:0 37:0 38:0 39:0 40:0")
    assert rows[b"not to {*} ."][1] == 5
    assert sum(r[1] for r in rows.values()) == 34 and len(rows) == 6


def test_restatement_by_hand():
    a, b, c, g = b"\x05", b"\x06", b"\x87\x01", b"\x03"
    sents = [[a, b, c], [], [a, c, c, a, b, c], [a, b], [c]]
    keys = [a + g + c, a + g + g + a, g + b + c, a + g + b]
    assert recount_all(keys, sents, 7) == {a + g + c: [(7, 0), (9, 0), (9, 3)], a + g + g + a: [(9, 0)], g + b + c: [(7, 0), (9, 3)], a + g + b: []}
    assert recount(keys, sents, 2) == {a + g + c: [(1, 0), (3, 0), (3, 3)], g + b + c: [(1, 0), (3, 3)]}


# ---- the C++ face, host route ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def recount_check(tmp_path_factory):
    exe = tmp_path_factory.mktemp("recount") / "recount_check"
    lib = os.path.join(PKG, "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(PKG, "host", "include"), "-I", os.path.join(ROOT, "include"), "-I", os.path.join(PKG, "csrc"),
                           os.path.join(ROOT, "tests", "recount_check.cpp"), os.path.join(lib, "libcolibri_amd_host.a"), "-L" + lib, "-lcolibri_hip", "-Wl,-rpath," + lib,
                           "-L/opt/rocm/lib", "-lrccl", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib", "-lpthread", "-o", str(exe)])
    return str(exe)


def face_rows(exe, corpus, kind, thr, first):
    out = subprocess.run([exe, os.path.join(COOC, f"{corpus}.is.colibri.patternmodel"), os.path.join(GOLDEN, corpus + ".colibri.dat"), kind, str(thr), str(first)],
                         capture_output=True, env=dict(os.environ, COLIBRI_RECOUNT="host"), timeout=300)
    assert out.returncode == 0, out.stderr.decode()
    lines = out.stdout.split(b"\n")
    rows = sorted((bytes.fromhex(c[0].decode()), int(c[1]), c[2] if len(c) > 2 else None) for c in (ln.split(b"\t") for ln in lines if b"\t" in ln))
    tail = [ln for ln in lines if ln.startswith(b"minmax")][0].split()
    return rows, (int(tail[1]), int(tail[2]), int(tail[4]))


@pytest.mark.parametrize("corpus", CORPORA)
@pytest.mark.parametrize("first", [1, 7])
def test_host_route_equals_the_restatement(recount_check, corpus, first):
    thr = 2
    keys = loaded_skipgrams(corpus, thr)
    found = recount(keys, corpus_sentences(corpus), thr, first)
    assert found
    for kind in ("i", "u"):
        rows, (minn, maxn, has) = face_rows(recount_check, corpus, kind, thr, first)
        assert rows == sorted((k, len(v), b" ".join(b"%d:%d" % r for r in v) if kind == "i" else None) for k, v in found.items()), (corpus, kind)
        lens = [len(key_tokens(k)) for k in found]
        assert minn <= min(lens) and maxn >= max(lens) and has == 1


def test_edge_is_pinned_to_the_restatement(recount_check):
    """edge (11 empty sentences among 69) at threshold 2: 18 skipgrams at 241 real token positions. The reference keeps the same 18 but finds
    154 of the 241 (a subset: its corpus iterator loses positions after empty sentences, tests/golden/recount/README.md), so edge has no fixture"""
    rows, _ = face_rows(recount_check, "edge", "u", 2, 1)
    found = recount(loaded_skipgrams("edge", 2), corpus_sentences("edge"), 2)
    assert len(rows) == len(found) == 18 and sum(r[1] for r in rows) == sum(len(v) for v in found.values()) == 241
    assert len([s for s in corpus_sentences("edge") if not s]) == 11 and len(corpus_sentences("edge")) == 69


def test_host_route_threshold_prunes_what_is_found_too_rarely(recount_check):
    """a threshold above a skipgram's stored count drops it at the load; none is found below the threshold afterwards"""
    rows, _ = face_rows(recount_check, "zipf20k", "i", 50, 1)
    assert [(k, c) for k, c, _ in rows] == sorted((k, len(v)) for k, v in recount(loaded_skipgrams("zipf20k", 50), corpus_sentences("zipf20k"), 50).items())
    assert len(rows) == 2


def test_abi_symbols_are_exported():
    from colibri_amd import capi
    L = capi.load()
    for name in ("colibri_recount", "colibri_recount_fetch", "colibri_recount_info"):
        assert name in capi.EXPORTED and getattr(L, name)
    assert L.colibri_abi_version() == 4
