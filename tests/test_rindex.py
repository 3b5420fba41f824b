"""The reverse index (colibri-patternmodeller -Z; PatternModel::getreverseindex / getreverseindex_bysentence / printreverseindex).

CPU part: a plain restatement of the specification (reference include/patternmodel.h:1746-1862, :2325-2338; the order is the defined one:
positions ascending, n ascending, the n-gram before its skipgrams, masks ascending), checked against the real reference's getreverseindex and
printreverseindex (tests/golden/rindex/, see the README there); the CLI's -Z on the host route against the restatement, byte for byte; the C++
face's getters. The GPU part (tests/test_gpu_rindex.py) holds the device against this restatement."""
import gzip
import os
import struct
import subprocess

import pytest

from conftest import GOLDEN, ROOT
from test_cooc import CLI, COOC, MODELS, key_tokens, sentences, skipmasks
from test_host_face import parse_model
from test_oracle import read_payload
from test_print import read_classes, text_of, tokens_of

RINDEX = os.path.join(GOLDEN, "rindex")
NGRAM, SKIPGRAM, FLEXGRAM = 1, 2, 3
# the filtered goldens: tag -> (occurrencecount, category, size)
FILTERS = {"o3": (3, 0, 0), "cN": (0, NGRAM, 0), "cS": (0, SKIPGRAM, 0), "s3": (0, 0, 3), "s3cS": (0, SKIPGRAM, 3)}
FILTERED = [("hamlet.v2", "is"), ("edge", "is")]
# the reference's own text is a golden only where the corpus has no empty sentence (its corpus iterator's numbering is an artefact there)
TEXT = [m for m in MODELS if os.path.exists(os.path.join(RINDEX, "printreverseindex.%s.%s.txt.gz" % m))]


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def reverse_index(counts, sents, occurrencecount=0, category=0, size=0, first_sentence=1):
    """getreverseindex(ref, occurrencecount, category, size) for every real token position: [(sentence, token, [keys in the defined order])]"""
    lens = [len(key_tokens(k)) for k in counts]
    minn, maxn = (min(lens), max(lens)) if lens else (1, 0)
    masks = skipmasks(counts)
    ok = lambda k: k in counts and (occurrencecount == 0 or counts[k] >= occurrencecount)
    out = []
    for s, toks in enumerate(sents):
        for t in range(len(toks)):
            keys = []
            for n in range(max(1, minn), min(maxn, len(toks) - t) + 1):
                if size and n != size:
                    continue
                w = toks[t:t + n]
                if category in (0, NGRAM) and ok(b"".join(w)):
                    keys.append(b"".join(w))
                if category in (NGRAM, FLEXGRAM) or n < 3:
                    continue
                for m in masks.get(n, ()):
                    mk = b"".join(b"\x03" if (m >> j) & 1 else w[j] for j in range(n))
                    if ok(mk):
                        keys.append(mk)
            out.append((first_sentence + s, t, keys))
    return out


def reverse_index_text(rows, words):
    """printreverseindex: "s:t", a tab and the text per pattern, a newline; one more newline after the last line"""
    return b"".join(b"%d:%d" % (s, t) + b"".join(b"\t" + text_of(tokens_of(k), words) for k in keys) + b"\n" for s, t, keys in rows) + b"\n"


def load(corpus, kind):
    _, _, _, counts, _ = parse_model(os.path.join(COOC, f"{corpus}.{kind}.colibri.patternmodel"))
    return counts, sentences(read_payload(corpus))


def golden_lines(name):
    with gzip.open(os.path.join(RINDEX, name), "rb") as f:
        return f.read().split(b"\n")


def as_golden(rows):
    return [b"%d:%d" % (s, t) + b"".join(b"\t" + k.hex().encode() for k in sorted(keys)) for s, t, keys in rows] + [b""]


def cls_for(corpus):
    return os.path.join(GOLDEN, "hamlet.colibri.cls" if corpus.startswith("hamlet") else "synthetic.colibri.cls")


def sort_fields(text):
    return [b"\t".join([l.split(b"\t")[0]] + sorted(l.split(b"\t")[1:])) for l in text.split(b"\n")]


def cli(args, **env):
    p = subprocess.run([CLI] + args, capture_output=True, env={**os.environ, **env}, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    return p.stdout, p.stderr.decode()


# ---- the restatement against the reference --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("corpus,kind", MODELS)
def test_restatement_equals_the_references_getreverseindex(corpus, kind):
    counts, sents = load(corpus, kind)
    assert as_golden(reverse_index(counts, sents)) == golden_lines(f"getreverseindex.{corpus}.{kind}.txt.gz")


@pytest.mark.parametrize("corpus,kind", FILTERED)
@pytest.mark.parametrize("tag", list(FILTERS))
def test_restatement_equals_the_references_filters(corpus, kind, tag):
    counts, sents = load(corpus, kind)
    occ, cat, size = FILTERS[tag]
    rows = reverse_index(counts, sents, occ, cat, size)
    assert as_golden(rows) == golden_lines(f"getreverseindex.{corpus}.{kind}.{tag}.txt.gz")
    assert reverse_index(counts, sents, 0, FLEXGRAM, 0) == [(s, t, []) for s, t, _ in rows]


def test_some_text_goldens_exist():
    assert TEXT and all(c in ("hamlet.v2", "edge", "zipf20k", "phrases15k") for c, _ in TEXT)


@pytest.mark.parametrize("corpus,kind", TEXT)
def test_restatement_text_equals_the_references_printreverseindex(corpus, kind):
    counts, sents = load(corpus, kind)
    assert all(sents), "text goldens are taken only from corpora without empty sentences"
    text = reverse_index_text(reverse_index(counts, sents), read_classes(cls_for(corpus)))
    with gzip.open(os.path.join(RINDEX, f"printreverseindex.{corpus}.{kind}.txt.gz"), "rb") as f:
        assert sort_fields(text) == sort_fields(f.read())


# ---- the CLI on the host route ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("corpus,kind", [(c, k) for c, k in MODELS if c in ("hamlet.v2", "edge")])
def test_cli_on_a_loaded_model(corpus, kind):
    counts, sents = load(corpus, kind)
    want = reverse_index_text(reverse_index(counts, sents), read_classes(cls_for(corpus)))
    args = ["-i", os.path.join(COOC, f"{corpus}.{kind}.colibri.patternmodel"), "-f", os.path.join(GOLDEN, f"{corpus}.colibri.dat"), "-c", cls_for(corpus), "-Z"]
    out, err = cli(args, COLIBRI_RINDEX="host")
    assert out == want and "on the device" not in err
    if (corpus, kind) in TEXT:
        with gzip.open(os.path.join(RINDEX, f"printreverseindex.{corpus}.{kind}.txt.gz"), "rb") as f:
            assert sort_fields(out) == sort_fields(f.read())


def write_unindexed(path, counts, tokens):
    """an unindexed model file: 00, type 10, version 2, tokens, types, patterns, then per pattern its key, 00 and its count"""
    raw = bytearray(b"\x00\x0a\x02") + struct.pack("<QQQ", tokens, 0, len(counts))
    for k, c in counts.items():
        raw += k + b"\x00" + struct.pack("<I", c)
    with open(path, "wb") as f:
        f.write(bytes(raw))


def test_cli_on_a_loaded_unindexed_model(tmp_path):
    """getreverseindex lives in the base model: an unindexed model over the loaded corpus prints the same index"""
    counts, sents = load("hamlet.v2", "is")
    path = str(tmp_path / "u.colibri.patternmodel")
    write_unindexed(path, counts, sum(len(s) for s in sents))
    want = reverse_index_text(reverse_index(counts, sents), read_classes(cls_for("hamlet.v2")))
    out, _ = cli(["-u", "-i", path, "-f", os.path.join(GOLDEN, "hamlet.v2.colibri.dat"), "-c", cls_for("hamlet.v2"), "-Z"], COLIBRI_RINDEX="host")
    assert out == want


def test_cli_on_a_model_without_unigrams(tmp_path):
    """minlength() is 2: a one-token sentence (shorter than minlength()) and every sentence's last token print their position alone; empty
    sentences are counted and print nothing"""
    counts, sents = load("edge", "is")
    counts = {k: c for k, c in counts.items() if len(key_tokens(k)) >= 2}
    assert any(len(s) == 1 for s in sents) and any(len(s) == 0 for s in sents)
    path = str(tmp_path / "m2.colibri.patternmodel")
    write_unindexed(path, counts, sum(len(s) for s in sents))
    rows = reverse_index(counts, sents)
    assert all(keys == [] for s, t, keys in rows if len(sents[s - 1]) == 1) and any(keys for _, _, keys in rows)
    out, _ = cli(["-u", "-i", path, "-f", os.path.join(GOLDEN, "edge.colibri.dat"), "-c", cls_for("edge"), "-Z"], COLIBRI_RINDEX="host")
    assert out == reverse_index_text(rows, read_classes(cls_for("edge")))


def test_cli_needs_a_class_file_and_a_corpus():
    model = os.path.join(COOC, "edge.i.colibri.patternmodel")
    p = subprocess.run([CLI, "-i", model, "-f", os.path.join(GOLDEN, "edge.colibri.dat"), "-Z"], capture_output=True, timeout=60)
    assert p.returncode == 2 and b"-Z needs a class file" in p.stderr
    p = subprocess.run([CLI, "-i", model, "-c", cls_for("edge"), "-Z"], capture_output=True, timeout=60)
    assert p.returncode == 2 and b"No corpus data file" in p.stderr


# ---- the C++ face --------------------------------------------------------------------------------------------------------------------------
CALLER = r"""
#include <algorithm>
#include <iostream>
#include "patternmodel.h"
static std::string hex(const PatternPointer& pp) {
    const Pattern p(pp);
    static const char* d = "0123456789abcdef";
    std::string s;
    for (size_t i = 0; i < p.bytesize(); ++i) { s += d[p.data[i] >> 4]; s += d[p.data[i] & 15]; }
    return s;
}
int main(int argc, char** argv) {
    IndexedCorpus corpus(argv[2]);
    PatternModelOptions opt;
    opt.MINTOKENS = 1; opt.DOSKIPGRAMS = true; opt.QUIET = true;
    IndexedPatternModel<> model(argv[1], opt, NULL, &corpus);
    const int occ = std::atoi(argv[3]), cat = std::atoi(argv[4]);
    const unsigned int size = (unsigned int)std::atoi(argv[5]);
    for (unsigned int s = 1; s <= corpus.sentences(); ++s) {
        const unsigned int sl = corpus.sentencelength((int)s);
        std::vector<std::vector<std::string>> by(sl);
        for (const auto& o : model.getreverseindex_bysentence((int)s, occ, cat, size)) {
            if (o.first.sentence != s || o.first.token >= sl) return 3;
            by[o.first.token].push_back(hex(o.second));
        }
        for (unsigned int t = 0; t < sl; ++t) {
            std::vector<std::string> keys;
            for (const PatternPointer& p : model.getreverseindex(IndexReference(s, (uint16_t)t), occ, cat, size)) keys.push_back(hex(p));
            std::sort(keys.begin(), keys.end());
            std::sort(by[t].begin(), by[t].end());
            if (keys != by[t]) return 4;
            std::cout << s << ":" << t;
            for (const std::string& k : keys) std::cout << "\t" << k;
            std::cout << "\n";
        }
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def caller(tmp_path_factory):
    d = tmp_path_factory.mktemp("rindex_caller")
    src, exe = d / "caller.cpp", d / "caller"
    src.write_text(CALLER)
    pkg = os.path.join(ROOT, "colibri-core_amd")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I" + os.path.join(pkg, "host", "include"), "-I" + os.path.join(ROOT, "include"), str(src),
                    os.path.join(pkg, "lib", "libcolibri_amd_host.a"), "-L" + os.path.join(pkg, "lib"), "-lcolibri_hip", "-Wl,-rpath," + os.path.join(pkg, "lib"), "-L/opt/rocm/lib", "-lrccl", "-lamdhip64",
                    "-Wl,-rpath,/opt/rocm/lib", "-lpthread", "-o", str(exe)], check=True, timeout=600)
    return str(exe)


@pytest.mark.parametrize("corpus,kind,tag", [(c, k, "") for c, k in MODELS if c in ("hamlet.v2", "edge")] + [(c, k, t) for c, k in FILTERED for t in FILTERS])
def test_cxx_getters_equal_the_references(caller, corpus, kind, tag):
    occ, cat, size = FILTERS.get(tag, (0, 0, 0))
    p = subprocess.run([caller, os.path.join(COOC, f"{corpus}.{kind}.colibri.patternmodel"), os.path.join(GOLDEN, f"{corpus}.colibri.dat"), str(occ), str(cat), str(size)],
                       capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    assert p.stdout.split(b"\n") == golden_lines(f"getreverseindex.{corpus}.{kind}{'.' + tag if tag else ''}.txt.gz")
