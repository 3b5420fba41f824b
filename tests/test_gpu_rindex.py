"""The reverse index on the device (colibri_rindex / colibri_rindex_resident / colibri_rindex_text; colibri-patternmodeller -Z under
COLIBRI_RINDEX), against the restatement of test_rindex.py: the arrays exactly, order included, and the text byte for byte."""
import os
import random

import numpy as np
import pytest

from conftest import GOLDEN
from test_cooc import COOC, MODELS, key_tokens, sentences
from test_gpu_coverage import varint
from test_host_face import parse_model
from test_oracle import read_payload
from test_print import read_classes
from test_rindex import FILTERED, FILTERS, cli, cls_for, load, reverse_index, reverse_index_text

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from colibri_amd import capi
    with capi.Context(0) as c:
        yield c


def arrays(keys):
    key_off = np.cumsum([0] + [len(k) for k in keys]).astype(np.uint64)
    return key_off, np.frombuffer(b"".join(keys) + b"\0", dtype=np.uint8)[:-1]


def rows_of(keys, fetched):
    pos_off, s, t, pat = fetched
    po, pat = [int(x) for x in pos_off], [int(x) for x in pat]
    assert len(po) == len(s) + 1 == len(t) + 1 and po[0] == 0 and po[-1] == len(pat)
    return [(int(s[r]), int(t[r]), [keys[p] for p in pat[po[r]:po[r + 1]]]) for r in range(len(s))]


def check(ctx, counts, sents, first=1, **flt):
    keys = list(counts)
    ko, kb = arrays(keys)
    got = rows_of(keys, ctx.reverse_index(ko, kb, np.array([counts[k] for k in keys], dtype=np.uint32), **flt))
    want = reverse_index(counts, sents, flt.get("occurrencecount", 0), flt.get("category", 0), flt.get("size", 0), first_sentence=first)
    assert got == want
    return want


# ---- the fixture models -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("corpus,kind", MODELS)
def test_uploaded_model_equals_the_restatement(ctx, corpus, kind):
    counts, sents = load(corpus, kind)
    ctx.upload(read_payload(corpus))
    check(ctx, counts, sents)
    check(ctx, counts, sents, occurrencecount=3, size=2)


@pytest.mark.parametrize("corpus,kind", MODELS)
def test_resident_model_equals_the_restatement(ctx, corpus, kind):
    small = corpus in ("hamlet.v2", "edge")
    payload = read_payload(corpus)
    ctx.upload(payload)
    ctx.train(mintokens=2 if small else 15, maxlength=4 if small else 3, indexed=int(kind != "u"), doskipgrams=int(kind == "is"))
    counts, _ = ctx.export_dict()
    key_off, key_bytes, _, _ = ctx.export_arrays()
    kb, off = key_bytes.tobytes(), key_off.tolist()
    keys = [kb[off[j]:off[j + 1]] for j in range(len(off) - 1)]
    sents = sentences(payload)
    for occ, cat, size in [(0, 0, 0), (3, 0, 0), (0, 2, 3)]:
        got = rows_of(keys, ctx.reverse_index(resident=True, occurrencecount=occ, category=cat, size=size))
        assert got == reverse_index(counts, sents, occ, cat, size)


def test_resident_unindexed_model(ctx):
    payload = read_payload("hamlet.v2")
    ctx.upload(payload)
    ctx.train(mintokens=2, maxlength=4, indexed=0)
    counts, _ = ctx.export_dict()
    key_off, key_bytes, _, _ = ctx.export_arrays()
    kb, off = key_bytes.tobytes(), key_off.tolist()
    keys = [kb[off[j]:off[j + 1]] for j in range(len(off) - 1)]
    assert rows_of(keys, ctx.reverse_index(resident=True, occurrencecount=3)) == reverse_index(counts, sentences(payload), 3)


@pytest.mark.parametrize("corpus,kind", FILTERED)
@pytest.mark.parametrize("tag", list(FILTERS))
def test_filters(ctx, corpus, kind, tag):
    counts, sents = load(corpus, kind)
    ctx.upload(read_payload(corpus))
    occ, cat, size = FILTERS[tag]
    check(ctx, counts, sents, occurrencecount=occ, category=cat, size=size)
    assert all(keys == [] for _, _, keys in check(ctx, counts, sents, category=3))


# ---- chunks and windows ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("corpus,kind", [("hamlet.v2", "is"), ("edge", "is")])
def test_chunks_cut_the_positions_anywhere(ctx, monkeypatch, corpus, kind):
    counts, sents = load(corpus, kind)
    ctx.upload(read_payload(corpus))
    npos = ctx.positions()
    for chunk in (None, 257, 64, 1):
        if chunk:
            monkeypatch.setenv("COLIBRI_RINDEX_CHUNK", str(chunk))
        check(ctx, counts, sents)
        chunks, _, _, scratch = ctx.reverse_index_info()
        assert chunks == (-(-npos // chunk) if chunk else 1) and scratch > 0, chunk


@pytest.mark.parametrize("corpus,kind", [("hamlet.v2", "is"), ("edge", "is")])
def test_windows_cut_lines_numbers_and_words_anywhere(ctx, monkeypatch, corpus, kind):
    counts, sents = load(corpus, kind)
    words = read_classes(cls_for(corpus))
    ctx.upload(read_payload(corpus))
    want = reverse_index_text(check(ctx, counts, sents), words)
    for window in (None, 7, 1):
        if window:
            monkeypatch.setenv("COLIBRI_RINDEX_WINDOW_BYTES", str(window))
        assert ctx.reverse_index_text(words) == want, window
        _, w, staging, _ = ctx.reverse_index_info()
        B = min(window or (64 << 20), len(want))
        assert w == -(-len(want) // B) and staging == 2 * B and ctx.rindex_bytes == len(want)


# ---- random corpora and models ---------------------------------------------------------------------------------------------------------------------
IDS = [5, 6, 7, 100, 127, 128, 129, 300, 16383, 16384, 16385, 20000]  # 1-, 2- and 3-byte tokens on both sides of 128 and 16384


def random_case(rnd, npos, variant):
    """a corpus of exactly npos positions (tokens and delimiters): empty and one-token sentences, where it fits a sentence of 300 tokens; a model
    of random windows of 2-5 tokens of it (no unigrams), skipgrams of windows whose n-gram is left out among them; a word table"""
    lens = [0, 1, 0, 1, 2] + ([300] if npos > 1000 else [])
    while sum(lens) + len(lens) < npos:
        lens.append(min(rnd.choice([0, 1, 2, 3, 5, 8, 13, 40]), npos - sum(lens) - len(lens) - 1))
    rnd.shuffle(lens)
    sents = [[varint(rnd.choice(IDS[:6] if rnd.random() < 0.7 else IDS)) for _ in range(n)] for n in lens]
    payload = b"".join(b"".join(s) + b"\x00" for s in sents)
    counts = {}
    for s in sents:
        for t in range(len(s)):
            for n in range(2, min(5, len(s) - t) + 1):
                w = s[t:t + n]
                if rnd.random() < 0.25:
                    counts[b"".join(w)] = rnd.randint(1, 5)
                if n >= 3 and rnd.random() < 0.15:  # (independent of the n-gram's draw: some skipgrams come without their n-gram)
                    gaps = rnd.sample(range(1, n - 1), rnd.randint(1, n - 2))
                    counts[b"".join(b"\x03" if j in gaps else w[j] for j in range(n))] = rnd.randint(1, 5)
    keys = list(counts)
    rnd.shuffle(keys)
    counts = {k: counts[k] for k in keys}
    words = {3: b"{*}", **{i: b"w%d" % i for i in IDS}}
    if variant == 1:
        del words[300], words[16384]  # ids without a word: {?}
    if variant == 2:
        words[5], words[128] = b"", b""  # a word that is the empty string
    return sents, payload, counts, words


@pytest.mark.parametrize("npos", [255, 256, 257, 4097])
@pytest.mark.parametrize("variant", [0, 1, 2])
def test_random_cases(ctx, monkeypatch, npos, variant):
    rnd = random.Random(1000 * npos + variant)
    sents, payload, counts, words = random_case(rnd, npos, variant)
    assert any(len(key_tokens(k)) >= 3 and b"\x03" in key_tokens(k) for k in counts) and min(len(key_tokens(k)) for k in counts) == 2
    first = 1 + 6 * (variant == 1)  # (a first-sentence offset above 1)
    ctx.upload(payload, first_sentence=first)
    assert ctx.positions() == npos
    monkeypatch.setenv("COLIBRI_RINDEX_CHUNK", "256")
    want = check(ctx, counts, sents, first)
    assert ctx.reverse_index_info()[0] == -(-npos // 256)
    monkeypatch.setenv("COLIBRI_RINDEX_WINDOW_BYTES", "4096")
    assert ctx.reverse_index_text(words) == reverse_index_text(want, words)
    monkeypatch.delenv("COLIBRI_RINDEX_CHUNK")
    check(ctx, counts, sents, first, occurrencecount=rnd.randint(2, 5), category=rnd.choice([0, 1, 2]), size=rnd.choice([0, 3, 4]))


# ---- the CLI --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("corpus,kind", [(c, k) for c, k in MODELS if c in ("hamlet.v2", "edge")])
def test_cli_device_route_equals_the_host_route(tmp_path, corpus, kind):
    dat, cls = os.path.join(GOLDEN, f"{corpus}.colibri.dat"), cls_for(corpus)
    loaded = ["-i", os.path.join(COOC, f"{corpus}.{kind}.colibri.patternmodel"), "-f", dat, "-c", cls, "-Z"]
    host, _ = cli(loaded, COLIBRI_RINDEX="host")
    out, err = cli(loaded, COLIBRI_RINDEX="device")
    assert out == host and "(reverse index on the device: uploaded model)" in err
    out, err = cli(loaded)  # auto: no break-even is set, nothing runs on the device
    assert out == host and "on the device" not in err
    # after training: an indexed skipgram model stays resident, the others are uploaded; -m 2: minlength() is 2
    for extra in ([], ["-m", "2"]):
        model = str(tmp_path / f"m{len(extra)}.colibri.patternmodel")
        train = ["-f", dat, "-c", cls, "-l", "4", "-t", "2", "-o", model, "-Z"] + (["-s"] if kind == "is" else []) + extra
        host, _ = cli(train, COLIBRI_RINDEX="host")
        _, _, _, counts, _ = parse_model(model)
        assert host == reverse_index_text(reverse_index(counts, sentences(read_payload(corpus))), read_classes(cls))
        out, err = cli(train, COLIBRI_RINDEX="device")
        form = "resident" if kind == "is" and not extra else "uploaded"
        assert out == host and f"(reverse index on the device: {form} model)" in err


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(ctx, monkeypatch):
    from colibri_amd import capi
    counts, sents = load("hamlet.v2", "is")
    ctx.upload(read_payload("hamlet.v2"))
    flex = dict(counts)
    flex[varint(5) + b"\x04" + varint(6)] = 2  # a flexgram
    ko, kb = arrays(list(flex))
    with pytest.raises(capi.ColibriError) as e:
        ctx.reverse_index(ko, kb)
    assert e.value.code == -4
    monkeypatch.setenv("COLIBRI_RINDEX_BUDGET", "1000")
    ko, kb = arrays(list(counts))
    with pytest.raises(capi.ColibriError) as e:
        ctx.reverse_index(ko, kb)
    assert e.value.code == -7
    with pytest.raises(capi.ColibriError) as e:
        ctx.reverse_index_text({})  # (no index stands after a refusal)
    assert e.value.code == -6
    monkeypatch.delenv("COLIBRI_RINDEX_BUDGET")
    check(ctx, counts, sents)


def test_state_errors():
    from colibri_amd import capi
    with capi.Context(0) as c:
        ko, kb = arrays([varint(5)])
        for call in (lambda: c.reverse_index(ko, kb), lambda: c.reverse_index(resident=True)):
            with pytest.raises(capi.ColibriError) as e:
                call()
            assert e.value.code == -6  # no corpus uploaded
        c.upload(read_payload("hamlet.v2"))
        with pytest.raises(capi.ColibriError) as e:
            c.reverse_index(resident=True)  # untrained
        assert e.value.code == -6
