"""print() with instances (colibri-patternmodeller -P --instantiate; colibri_print_instances, csrc/print.hpp), without a device: a restatement of the rows on
top of test_print.print_rows, checked against the text the reference's own print(cout, decoder, true) wrote for three models (tests/golden/instantiate/), the
CLI's host loop against the same text, its refusals, the look-up header under the sanitizers, and the presence of the new entry points.
test_gpu_instantiate.py holds the device to this restatement."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from test_coverage import category_of, tokens_of
from test_print import print_rows, read_classes, text_of
from test_views import CLI, GOLD, ROOT, VIEWS, golden

INST = os.path.join(GOLD, "instantiate")
FIXTURES = {  # fixture -> (corpus, class file): the reference's print(cout, decoder, true) of the model it trained with DOSKIPGRAMS (README.md there)
    "hamlet.v2": ("hamlet.v2", "hamlet.colibri.cls"),
    "edge": ("edge", "synthetic.colibri.cls"),
    "zipf20k": ("zipf20k", "synthetic.colibri.cls"),
}
HEADER = b"PATTERN\tCOUNT\tTOKENS\tCOVERAGE\tCATEGORY\tSIZE\tFREQUENCY\tREFERENCES"


def sentences_of(corpus):
    """the sentences of a v2 payload (no header) as lists of class ids: every delimiter ends one, empty ones included"""
    out, cur = [], []
    for t in tokens_of(bytes(corpus)):
        if t == 0:
            out.append(cur)
            cur = []
        else:
            cur.append(t)
    return out + [cur]


def instance_rows(words, arrays, tokens, corpus, first_sentence=1):
    """the rows of print(out, decoder, true) of an indexed model over its corpus: print_rows, and in a skipgram row every reference s:t is followed by
    [ the words of the n corpus tokens from (s, t) on ]. ValueError for a flexgram in the model and for a reference whose window is not in the corpus."""
    key_off, key_bytes, counts, refs = arrays
    rows = print_rows(words, arrays, tokens)
    if refs is None:
        return rows
    kb, off = bytes(bytearray(np.asarray(key_bytes, dtype=np.uint8).tolist())), [int(x) for x in key_off]
    toks = [tokens_of(kb[off[j]:off[j + 1]]) for j in range(len(off) - 1)]
    if any(category_of(t) == 3 for t in toks):
        raise ValueError("flexgram")
    sent = sentences_of(corpus)
    ro, rs, rt = ([int(x) for x in a] for a in refs)
    for j, t in enumerate(toks):
        if category_of(t) != 2:
            continue
        parts = []
        for r in range(ro[j], ro[j + 1]):
            s = rs[r] - first_sentence
            if s < 0 or s >= len(sent) or rt[r] + len(t) > len(sent[s]):
                raise ValueError("does not fit")
            parts.append(b"%d:%d[%s]" % (rs[r], rt[r], text_of(sent[s][rt[r]:rt[r] + len(t)], words)))
        rows[j] = rows[j][: rows[j].rindex(b"\t") + 1] + b" ".join(parts) + b"\n"
    return rows


def fixture_text(name):
    path = os.path.join(INST, f"{name}.print.txt")
    return open(path, "rb").read() if os.path.exists(path) else gzip.open(path + ".gz", "rb").read()


def fixture_case(name):
    """(words, arrays, tokens, corpus payload) of a fixture's model file and corpus"""
    from colibri_amd import digest
    corpus, cls = FIXTURES[name]
    mtype, tokens, types, key_off, key_bytes, counts, refs = digest.parse_model_file(os.path.join(INST, f"{name}.colibri.patternmodel"))
    assert mtype == 20
    payload = open(os.path.join(GOLD, f"{corpus}.colibri.dat"), "rb").read()[2:]  # (behind the two header bytes)
    return read_classes(os.path.join(GOLD, cls)), (key_off, key_bytes, None, refs), int(tokens), payload


def same_rows(out, want):
    got_lines, want_lines = out.split(b"\n"), want.split(b"\n")
    assert got_lines[0] == want_lines[0]
    assert sorted(got_lines[1:]) == sorted(want_lines[1:])


def run_cli(args, mode="host"):
    return subprocess.run([CLI] + args, capture_output=True, env={**os.environ, "COLIBRI_PRINT": mode}, timeout=300)


def cli_args(name, corpus=True):
    c, cls = FIXTURES[name]
    return ["-i", os.path.join(INST, f"{name}.colibri.patternmodel"), "-c", os.path.join(GOLD, cls)] + (["-f", os.path.join(GOLD, f"{c}.colibri.dat")] if corpus else [])


@pytest.mark.parametrize("name", list(FIXTURES))
def test_restatement_reproduces_the_reference_text(name):
    words, arrays, tokens, payload = fixture_case(name)
    want = fixture_text(name)
    assert want.split(b"\n")[0] == HEADER and want.count(b"skipgram") >= 6 and want.count(b"[") >= 12
    same_rows(HEADER + b"\n" + b"".join(instance_rows(words, arrays, tokens, payload)), want)


def test_restatement_on_a_model_written_by_hand():
    """an empty word leaves no space behind it, an id without a word prints {?}, the gaps' fillers need not be patterns, sentences are numbered from
    first_sentence with the empty one counted, an n-gram row stays as it is; a window one token too long, a sentence the corpus lacks and a flexgram are refused"""
    words = {5: b"", 6: b"b", 7: b"cc", 3: b"GAP", 4: b"{**}", 300: b"far"}
    corpus = b"\x06\x05\x07\x00\x00\x05\xac\x02\x08\x06"  # 6 5 7 | (empty) | 5 300 8 6
    keys = [b"\x06\x03\x07", b"\x06", b"\x05\x03\x03\x06"]
    refs = [[(5, 0)], [(5, 0), (7, 3)], [(7, 0)]]
    key_off = np.cumsum([0] + [len(k) for k in keys]).astype(np.uint64)
    model = lambda refs: (key_off, np.frombuffer(b"".join(keys), dtype=np.uint8), None,
                          (np.cumsum([0] + [len(r) for r in refs]).astype(np.uint64), np.array([s for r in refs for s, _ in r], dtype=np.uint32),
                           np.array([t for r in refs for _, t in r], dtype=np.uint16)))
    assert instance_rows(words, model(refs), 10, corpus, 5) == [
        b"b GAP cc\t1\t3\t0.3\tskipgram\t3\t1\t5:0[b  cc]\n",
        b"b\t2\t2\t0.2\tngram\t1\t1\t5:0 7:3\n",
        b"GAP GAP b\t1\t4\t0.4\tskipgram\t4\t1\t7:0[far {?} b]\n",
    ]
    for bad in ([[(5, 1)], [], []], [[(6, 0)], [], []], [[(8, 0)], [], []], [[(4, 0)], [], []], [[], [], [(7, 1)]]):
        with pytest.raises(ValueError):
            instance_rows(words, model(bad), 10, corpus, 5)
    flex = (np.array([0, 3], dtype=np.uint64), np.frombuffer(b"\x06\x04\x07", dtype=np.uint8), None,
            (np.array([0, 1], dtype=np.uint64), np.array([5], dtype=np.uint32), np.array([0], dtype=np.uint16)))
    with pytest.raises(ValueError):
        instance_rows(words, flex, 10, corpus, 5)


@pytest.mark.parametrize("name", list(FIXTURES))
def test_cli_host_loop_equals_the_reference_text(name):
    p = run_cli(cli_args(name) + ["-P", "--instantiate"])
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    same_rows(p.stdout, fixture_text(name))
    assert b"on the device" not in p.stderr


def test_cli_without_a_corpus_or_unindexed_prints_plain():
    plain = run_cli(cli_args("hamlet.v2", corpus=False) + ["-P"])
    assert plain.returncode == 0 and b"[" not in plain.stdout and plain.stdout.count(b"skipgram") == 6
    p = run_cli(cli_args("hamlet.v2", corpus=False) + ["-P", "--instantiate"])  # no corpus attached: as in the reference
    assert p.returncode == 0 and p.stdout == plain.stdout
    # the golden print of the views' own indexed skipgram model, with and without the option
    views = ["-i", os.path.join(VIEWS, "hamlet.is.colibri.patternmodel"), "-c", os.path.join(GOLD, "hamlet.colibri.cls")]
    p = run_cli(views + ["-P", "--instantiate"])
    assert p.returncode == 0
    same_rows(p.stdout, golden("hamlet.is", "print"))
    # an unindexed model: unchanged, with the corpus given too
    un = ["-i", os.path.join(VIEWS, "hamlet.us.colibri.patternmodel"), "-c", os.path.join(GOLD, "hamlet.colibri.cls"), "-u"]
    p = run_cli(un + ["-P", "--instantiate", "-f", os.path.join(GOLD, "hamlet.v2.colibri.dat")])
    assert p.returncode == 0
    same_rows(p.stdout, golden("hamlet.us", "print"))


def test_cli_refuses_a_flexgram_before_any_byte():
    args = ["-i", os.path.join(INST, "hamlet.v2.flex.colibri.patternmodel"), "-c", os.path.join(GOLD, "hamlet.colibri.cls")]
    plain = run_cli(args + ["-P"])
    assert plain.returncode == 0 and plain.stdout.count(b"\tflexgram\t") == 6
    p = run_cli(args + ["-f", os.path.join(GOLD, "hamlet.v2.colibri.dat"), "-P", "--instantiate"])
    assert p.returncode != 0 and p.stdout == b"" and b"flexgrams, which are not instantiated" in p.stderr


def test_cli_refuses_a_model_beside_a_shorter_corpus_before_any_byte():
    c, cls = FIXTURES["zipf20k"]
    p = run_cli(cli_args("zipf20k", corpus=False) + ["-f", os.path.join(GOLD, "hamlet.v2.colibri.dat"), "-P", "--instantiate"])
    assert p.returncode != 0 and p.stdout == b"" and b"does not fit the corpus" in p.stderr


def test_instance_window_under_the_sanitizers(tmp_path):
    """host/include/instance_window.h under AddressSanitizer and UBSan on payloads held in heap blocks of exactly their size: windows at a sentence's first and last
    token, one token too long, a sentence beyond the corpus, an empty sentence, first_sentence > 1, multi-byte class ids (tests/instance_window_check.cpp holds the cases)"""
    exe = tmp_path / "instance_window_check"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "colibri-core_amd", "host", "include"),
                           os.path.join(ROOT, "tests", "instance_window_check.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.split()[0] == "checked" and int(out.stdout.split()[1]) >= 20 and out.stdout.split()[3] == "0"


def test_the_header_the_library_and_the_python_face_have_the_instance_calls():
    import inspect
    from colibri_amd import capi
    header = open(os.path.join(ROOT, "include", "colibri_hip.h")).read()
    assert "int colibri_print_instances(colibri_ctx* ctx," in header and "int colibri_print_instances_resident(colibri_ctx* ctx," in header
    assert "#define COLIBRI_ABI_VERSION 4 " in header
    L = capi.load()
    assert L.colibri_abi_version() == 4
    for name in ("colibri_print_instances", "colibri_print_instances_resident"):
        assert name in capi.EXPORTED and hasattr(L, name)
    assert inspect.signature(capi.Context.print_model).parameters["instantiate"].default is False
