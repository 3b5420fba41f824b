"""The skipgrams of an in-place rebuild on the device (colibri_recount / _fetch / _info; colibri-patternmodeller -I -s under COLIBRI_RECOUNT),
against the restatement of test_recount.py: counts and reference lists exactly; the CLI's text against what the reference printed."""
import os
import random
import struct
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN
from test_cooc import BIN, CLI, COOC, key_tokens, load_model
from test_gpu_coverage import varint
from test_oracle import read_payload
from test_print import read_classes
from test_recount import CORPORA, FIXTURES, corpus_sentences, fixture_text, loaded_skipgrams, recount, recount_all, restated_rows, skipgram_rows
from test_rindex import cli, cls_for

pytestmark = pytest.mark.gpu

UNSUPPORTED, STATE, OVERFLOW = -4, -6, -7
GAP = b"\x03"


@pytest.fixture(scope="module")
def ctx():
    from colibri_amd import capi
    with capi.Context(0) as c:
        yield c


def arrays(keys):
    key_off = np.cumsum([0] + [len(k) for k in keys]).astype(np.uint64)
    return key_off, np.frombuffer(b"".join(keys) + b"\0", dtype=np.uint8)[:-1]


def check(ctx, keys, sents, first=1, indexed=1, mintokens=1):
    """one recount of keys on the uploaded corpus against the restatement; returns the restatement's {key: references}"""
    ko, kb = arrays(keys)
    counts, ref_off, rs, rt = ctx.recount(ko, kb, indexed=indexed, mintokens=mintokens)
    want = recount_all(keys, sents, first)
    assert [int(c) for c in counts] == [len(want[k]) for k in keys]
    assert ctx.recount_kept == sum(1 for k in keys if len(want[k]) >= mintokens)
    if not indexed:
        assert ref_off is None and len(rs) == 0 and len(rt) == 0
        return want
    ro = [int(x) for x in ref_off]
    assert len(ro) == len(keys) + 1 and ro[0] == 0 and ro[-1] == len(rs) == len(rt)
    for j, k in enumerate(keys):
        got = list(zip((int(x) for x in rs[ro[j]:ro[j + 1]]), (int(x) for x in rt[ro[j]:ro[j + 1]])))
        assert got == (want[k] if len(want[k]) >= mintokens else []), k.hex()
    return want


# ---- the fixture models -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("corpus", CORPORA)
@pytest.mark.parametrize("indexed", [1, 0])
def test_fixture_models_equal_the_restatement(ctx, corpus, indexed):
    keys = loaded_skipgrams(corpus, 0)
    sents = corpus_sentences(corpus)
    ctx.upload(read_payload(corpus))
    want = check(ctx, keys, sents, indexed=indexed, mintokens=1)
    check(ctx, keys, sents, indexed=indexed, mintokens=2)
    above = max(len(v) for v in want.values()) + 1
    check(ctx, keys, sents, indexed=indexed, mintokens=above)  # everything empty
    assert ctx.recount_kept == 0
    groups, chunks, scratch = ctx.recount_info()
    assert groups == len({(len(key_tokens(k)), tuple(i for i, t in enumerate(key_tokens(k)) if t == GAP)) for k in keys}) and chunks == 1 and scratch > 0


# ---- crafted corpora ------------------------------------------------------------------------------------------------------------------------------
A, B, C, D, E = varint(5), varint(6), varint(200), varint(20000), varint(3000000)  # class ids of 1, 1, 2, 3 and 4 bytes
LONG = [varint(10 + i) for i in range(14)]


def crafted():
    """a corpus of a few hundred tokens: the edge sentences first, then random ones over the same ids"""
    assert [len(x) for x in (A, C, D, E)] == [1, 2, 3, 4]
    rnd = random.Random(20)
    sents = [[A, B, C],                    # 1: A {*} C ends exactly at the sentence end
             [A, B],                       # 2: one token short of fitting; the fixed token C stands just past the sentence end
             [C],                          # 3: one token
             [],                           # 4: none
             [A, B],                       # 5: two
             [A, D, C, E, A, C, C, E, B],  # 6: multi-byte ids in fixed and in gap positions; a window that two masks of one length match
             LONG,                         # 7: fourteen tokens: the 13-token skipgram fits at 0, with a token to spare
             LONG[:13],                    # 8: thirteen: it fits at 0 only, ending exactly at the end
             LONG[:12]]                    # 9: twelve: it does not fit
    pool = [A, A, B, C, C, D, E]
    while sum(len(s) + 1 for s in sents) < 600:
        sents.append([rnd.choice(pool) for _ in range(rnd.choice([0, 1, 2, 3, 4, 7, 12]))])
    payload = b"".join(b"".join(s) + b"\x00" for s in sents)
    return sents, payload


def join(*toks):
    return b"".join(toks)


CRAFTED_KEYS = [
    join(A, GAP, C),              # mask 010 at length 3 ...
    join(A, GAP, C, E),           # ... and at length 4
    join(A, D, GAP, E),           # same length and first word as the one above, another mask: both match sentence 6 at 0
    join(A, GAP, GAP, E),
    join(D, GAP, E),              # 3- and 4-byte ids fixed, a 2-byte id in the gap
    join(C, GAP, A),              # a 4-byte id in the gap
    join(A, GAP, B),              # (the random sentences decide what fills it)
    join(C, GAP, E, B),
    join(E, GAP, C, GAP, E),      # two gaps
    join(*(LONG[:6] + [GAP] + LONG[7:13])),  # exactly 13 tokens
    join(B, GAP, varint(9999)),   # occurs nowhere
]


@pytest.mark.parametrize("first", [1, 7])
@pytest.mark.parametrize("indexed", [1, 0])
def test_crafted_corpus(ctx, first, indexed):
    sents, payload = crafted()
    ctx.upload(payload, first_sentence=first)
    want = check(ctx, CRAFTED_KEYS, sents, first, indexed)
    f = first
    assert [r for r in want[join(A, GAP, C)] if r[0] < f + 6] == [(f, 0), (f + 5, 0), (f + 5, 4)]  # not at sentence 2 (C is the next sentence's); over a 3- and a 2-byte gap
    assert [r for r in want[join(A, GAP, C, E)] if r[0] < f + 6] == [(f + 5, 0), (f + 5, 4)]
    assert [r for r in want[join(A, D, GAP, E)] if r[0] < f + 6] == [(f + 5, 0)]
    assert [r for r in want[CRAFTED_KEYS[9]] if r[0] < f + 9] == [(f + 6, 0), (f + 7, 0)]
    assert want[CRAFTED_KEYS[10]] == []
    check(ctx, CRAFTED_KEYS, sents, first, indexed, mintokens=2)
    check(ctx, CRAFTED_KEYS[::-1], sents, first, indexed, mintokens=3)  # (the order of the keys is the caller's)


def test_zero_keys(ctx):
    sents, payload = crafted()
    ctx.upload(payload)
    counts, ref_off, rs, rt = ctx.recount(np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint8)[:0])
    assert len(counts) == 0 and [int(x) for x in ref_off] == [0] and len(rs) == 0 and ctx.recount_kept == 0


def test_refusals_leave_the_context_usable(ctx, monkeypatch):
    from colibri_amd import capi
    sents, payload = crafted()
    ctx.upload(payload)
    bad = {"fourteen tokens": join(*(LONG[:6] + [GAP] + LONG[7:14])), "an n-gram": join(A, B, C), "a flexgram": join(A, b"\x04", C), "two tokens": join(A, GAP),
           "a gap beside a flexgram gap": join(A, GAP, b"\x04", C)}
    for what, key in bad.items():
        ko, kb = arrays(CRAFTED_KEYS[:3] + [key])
        with pytest.raises(capi.ColibriError) as e:
            ctx.recount(ko, kb)
        assert e.value.code == UNSUPPORTED, what
        check(ctx, CRAFTED_KEYS, sents)  # the context serves the next call
    monkeypatch.setenv("COLIBRI_RECOUNT_BUDGET", "1000")
    ko, kb = arrays(CRAFTED_KEYS)
    with pytest.raises(capi.ColibriError) as e:
        ctx.recount(ko, kb)
    assert e.value.code == OVERFLOW
    assert ctx.L.colibri_recount_fetch(ctx.h, None, None, None, None) == STATE  # (no result stands after a refusal)
    monkeypatch.delenv("COLIBRI_RECOUNT_BUDGET")
    check(ctx, CRAFTED_KEYS, sents)


def test_state_error_without_a_corpus():
    from colibri_amd import capi
    with capi.Context(0) as c:
        ko, kb = arrays(CRAFTED_KEYS)
        with pytest.raises(capi.ColibriError) as e:
            c.recount(ko, kb)
        assert e.value.code == STATE


# ---- chunks ---------------------------------------------------------------------------------------------------------------------------------------
def test_references_span_chunks_and_ascend(ctx, monkeypatch):
    keys = loaded_skipgrams("phrases15k", 0)
    sents = corpus_sentences("phrases15k")
    ctx.upload(read_payload("phrases15k"))
    npos = ctx.positions()
    chunk = 5000
    assert npos > 2 * chunk
    monkeypatch.setenv("COLIBRI_RECOUNT_CHUNK", str(chunk))
    want = check(ctx, keys, sents)
    _, chunks, _ = ctx.recount_info()
    assert chunks == -(-npos // chunk) >= 3
    # one pattern's references come from every chunk: positions before the first cut and after the last
    firsts = np.cumsum([0] + [len(s) + 1 for s in sents])
    pos = [int(firsts[s - 1]) + t for s, t in max(want.values(), key=len)]
    assert pos == sorted(pos) and {p // chunk for p in pos} == set(range(chunks))


@pytest.mark.parametrize("chunk", [1, 64, 257])
def test_chunks_cut_windows_anywhere(ctx, monkeypatch, chunk):
    sents, payload = crafted()
    ctx.upload(payload)
    monkeypatch.setenv("COLIBRI_RECOUNT_CHUNK", str(chunk))
    check(ctx, CRAFTED_KEYS, sents, mintokens=2)
    assert ctx.recount_info()[1] == -(-ctx.positions() // chunk)


# ---- the CLI and the face, end to end ---------------------------------------------------------------------------------------------------------------
def rebuild_args(corpus, kind, thr, model=None, maxlen=None):
    maxlen = maxlen or ("4" if corpus in ("hamlet.v2", "edge") else "3")  # (what the fixture models were trained with; the load drops what is longer)
    return (["-u"] if kind == "u" else []) + ["-I", "-i", model or os.path.join(COOC, f"{corpus}.is.colibri.patternmodel"), "-f", os.path.join(GOLDEN, corpus + ".colibri.dat"), "-s",
                                               "-t", str(thr), "-l", maxlen, "-c", cls_for(corpus), "-P"]


@pytest.mark.parametrize("corpus", sorted(FIXTURES))
@pytest.mark.parametrize("kind", ["i", "u"])
@pytest.mark.parametrize("route", ["device", "host"])
def test_cli_rebuild_equals_the_reference(corpus, kind, route):
    want = fixture_text(corpus, kind, 2)
    out, err = cli(rebuild_args(corpus, kind, 2), COLIBRI_RECOUNT=route)
    assert sorted(out.split(b"\n")) == sorted(want.split(b"\n"))
    found = sum(r[1] for r in skipgram_rows(want))
    assert "Finding skipgrams/flexgrams matching preloaded constraints, occurrence threshold 2 ..." in err
    assert f" Found {found} skipgrams, 0 flexgrams ... pruned 0" in err
    assert ("(skipgram recount on the device: resident corpus)" in err) == (route == "device")


@pytest.mark.parametrize("corpus", sorted(FIXTURES))
def test_cli_threshold_that_drops_skipgrams_at_the_load(corpus):
    thr = FIXTURES[corpus][1][1]
    for kind in ("i", "u"):
        out, err = cli(rebuild_args(corpus, kind, thr))  # auto: the device
        assert sorted(out.split(b"\n")) == sorted(fixture_text(corpus, kind, thr).split(b"\n"))
        assert (" None found" in err) == (not skipgram_rows(out))


def test_cli_edge_equals_the_restatement():
    words = read_classes(cls_for("edge"))
    found = recount(loaded_skipgrams("edge", 2), corpus_sentences("edge"), 2)
    for kind in ("i", "u"):
        for route in ("device", "host"):
            out, _ = cli(rebuild_args("edge", kind, 2), COLIBRI_RECOUNT=route)
            assert skipgram_rows(out) == restated_rows(found, words, kind == "i"), (kind, route)


def test_pattern_list_with_gaps_counts_where_the_patterns_fit(tmp_path):
    """a list of patterns, gaps included, becomes a model with -L; -I -s -t 1 then counts every one of them on the corpus (what colibri-findpatterns wraps)"""
    cls = cls_for("hamlet.v2")
    lines = [b"To {*} or", b"to be", b"not to {*} .", b"be {*} {*} to", b"or", b"To {*} {*} not {*} be", b"question {*} To"]
    (tmp_path / "list.txt").write_bytes(b"\n".join(lines) + b"\n")
    r = subprocess.run([os.path.join(BIN, "colibri-classencode"), "-c", cls, "-e", "-o", "list", "list.txt"], cwd=tmp_path, capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()
    model = str(tmp_path / "list.colibri.patternmodel")
    cli(["-L", "-f", str(tmp_path / "list.colibri.dat"), "-o", model])
    out, err = cli(rebuild_args("hamlet.v2", "i", 1, model, maxlen="6"))
    ids = {w: k for k, w in read_classes(cls).items()}
    sents = corpus_sentences("hamlet.v2")
    want = []
    for ln in lines:
        toks = [varint(ids[w]) for w in ln.split(b" ")]
        if GAP in toks:
            refs = recount_all([b"".join(toks)], sents)[b"".join(toks)]
        else:
            refs = [(s + 1, t) for s, sent in enumerate(sents) for t in range(len(sent) - len(toks) + 1) if sent[t:t + len(toks)] == toks]
        if refs:
            want.append((ln, len(refs), b" ".join(b"%d:%d" % x for x in refs)))
    got = sorted((c[0], int(c[1]), c[7].strip()) for c in (ln.split(b"\t") for ln in out.split(b"\n")) if len(c) > 7 and c[0] != b"PATTERN")
    assert got == sorted(want) and len(want) >= 5 and any(b"{*}" in w[0] and w[1] > 1 for w in want)


def write_unindexed_model(path, counts, tokens, types):
    with open(path, "wb") as f:
        f.write(b"\x00\x0a\x02" + struct.pack("<QQQ", tokens, types, len(counts)))
        for k, c in counts.items():
            f.write(k + b"\x00" + struct.pack("<I", c))


def test_a_model_holding_a_flexgram_is_refused(tmp_path):
    counts, _ = load_model("hamlet.v2", "is")
    counts = dict(counts)
    counts[join(varint(11), b"\x04", varint(12))] = 4
    model = str(tmp_path / "flex.colibri.patternmodel")
    write_unindexed_model(model, counts, 354, 100)
    for kind in ("i", "u"):
        p = subprocess.run([CLI] + rebuild_args("hamlet.v2", kind, 2, model), capture_output=True, timeout=300)
        assert p.returncode != 0 and b"the loaded model holds flexgrams" in p.stderr and b"skipgram\t" not in p.stdout
