"""print() with instances on the device (colibri_print_instances; colibri-patternmodeller -P --instantiate under COLIBRI_PRINT=device), against the restatement
of test_instantiate.py and the reference's own text in tests/golden/instantiate/. Every comparison is of bytes."""
import os
import random
import subprocess

import numpy as np
import pytest

from test_gpu_coverage import flat, varint
from test_instantiate import FIXTURES, cli_args, fixture_case, fixture_text, instance_rows, same_rows
from test_print import print_rows
from test_views import CLI, GOLD

pytestmark = pytest.mark.gpu
TRAIN = {"hamlet.v2": ["-s", "-t", "2", "-l", "4"], "edge": ["-s", "-t", "2", "-l", "4", "-T", "1"], "zipf20k": ["-s", "-t", "5", "-l", "3"]}  # as the fixtures were trained


@pytest.fixture(scope="module")
def ctx():
    from colibri_amd import capi
    with capi.Context(0) as c:
        yield c


def cli(args):
    p = subprocess.run([CLI] + args, capture_output=True, env={**os.environ, "COLIBRI_PRINT": "device"}, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    return p.stdout, p.stderr.decode()


# ---- the reference's text ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(FIXTURES))
def test_fixtures_uploaded_and_resident(ctx, name):
    words, arrays, tokens, payload = fixture_case(name)
    want = b"".join(instance_rows(words, arrays, tokens, payload))
    ctx.upload(payload)
    assert ctx.print_model(words, arrays, tokens, instantiate=True) == want
    assert ctx.print_bytes == len(want)
    # a loaded model beside its corpus: the uploaded form
    out, err = cli(cli_args(name) + ["-P", "--instantiate"])
    same_rows(out, fixture_text(name))
    assert "(print on the device: uploaded model, instances)" in err
    # a training run leaves model and corpus in HBM: the resident form
    corpus, cls = FIXTURES[name]
    out, err = cli(["-f", os.path.join(GOLD, f"{corpus}.colibri.dat"), "-c", os.path.join(GOLD, cls)] + TRAIN[name] + ["-P", "--instantiate"])
    same_rows(out, fixture_text(name))
    assert "(print on the device: resident model, instances)" in err
    # without the corpus the rows are plain, on the device too
    out, err = cli(cli_args(name, corpus=False) + ["-P", "--instantiate"])
    assert b"[" not in out and "(print on the device: uploaded model)" in err


# ---- windows -----------------------------------------------------------------------------------------------------------------------------------
def test_windows_cut_instances_anywhere(ctx, monkeypatch):
    words, arrays, tokens, payload = fixture_case("hamlet.v2")
    want = b"".join(instance_rows(words, arrays, tokens, payload))
    ctx.upload(payload)
    for window in (None, 7, 1):
        if window:
            monkeypatch.setenv("COLIBRI_PRINT_WINDOW_BYTES", str(window))
        assert ctx.print_model(words, arrays, tokens, instantiate=True) == want, window
        w, staging, scratch = ctx.print_info()
        B = min(window or (64 << 20), len(want))
        assert w == -(-len(want) // B) and staging == 2 * B and scratch > 0 and ctx.print_bytes == len(want)
        assert ctx.print_model(words, arrays, tokens, instantiate=False) == b"".join(print_rows(words, arrays, tokens)), window  # the new argument, off: today's bytes


# ---- balance -----------------------------------------------------------------------------------------------------------------------------------
def test_a_head_skipgram_across_slices(ctx, monkeypatch):
    """one skipgram of 5 000 references among 50 small patterns, n-gram and skipgram rows in turn, 64 references per slice and windows of 4 096 bytes: slice and
    window bounds fall inside rows of both kinds"""
    rnd = random.Random(7)
    sents = [[rnd.randint(6, 60) for _ in range(rnd.randint(3, 14))] for _ in range(700)]
    payload = b"".join(b"".join(varint(t) for t in s) + b"\x00" for s in sents)
    place = lambda n: next((s + 1, rnd.randint(0, len(sents[s]) - n)) for s in iter(lambda: rnd.randrange(len(sents)), None) if len(sents[s]) >= n)
    refs = {}
    for i in range(1, 51):
        key = varint(6 + i) if i % 2 else varint(6 + i) + b"\x03" + varint(7 + i)
        refs[key] = [place(3) for _ in range(rnd.randint(0, 30))]
    refs[varint(30) + b"\x03\x03" + varint(7)] = [place(4) for _ in range(5000)]
    key_off, kb, _, r = flat(refs)
    arrays = (key_off, kb, None, r)
    words = {6 + i: b"w%d" % i for i in range(60)}
    want = b"".join(instance_rows(words, arrays, 123457, payload))
    assert want.count(b"\tskipgram\t") == 26 and want.count(b"[") > 5000
    monkeypatch.setenv("COLIBRI_PRINT_SLICE", "64")
    monkeypatch.setenv("COLIBRI_PRINT_WINDOW_BYTES", "4096")
    ctx.upload(payload)
    assert ctx.print_model(words, arrays, 123457, instantiate=True) == want
    assert ctx.print_info()[0] == -(-len(want) // 4096) > 10


# ---- random models -----------------------------------------------------------------------------------------------------------------------------
IDS = [5, 6, 7, 8, 127, 128, 300, 20000, 2 ** 21 - 1, 2 ** 21 + 7]


def random_instance_case(rnd):
    """(words, arrays, tokens, payload, first_sentence, features): a corpus of at most 200 tokens with sentences of 0, 1, n and n + 1 tokens around a skipgram length n,
    ids 5 .. 2^21 + 7 with words missing, empty and multi-byte (test_gpu_print.random_print_model's table), a redefined class 3, skipgrams of 3 .. 13 tokens with one gap
    behind the first token (trailing content), one before the last (leading content) or several, references at a sentence's last fitting token, n-grams between them"""
    words = {3: rnd.choice([b"{*}", b"GAP"]), 4: b"{**}", 5: b"", 6: b"b", 7: b"cc", 127: b"edge", 128: b"two", 20000: b"three", 2 ** 21 - 1: "été".encode()}  # 8, 300, 2^21 + 7: no word
    first = rnd.choice([1, 5])
    n0 = rnd.randint(3, 13)
    lengths = [0, 1, n0, n0 + 1] + [rnd.choice([0, 1, 2, 3, 5, 8, 13, 14, 20]) for _ in range(rnd.randint(0, 8))]
    rnd.shuffle(lengths)
    sents, total = [], 0
    for n in lengths:
        if total + n > 200:
            continue
        sents.append([rnd.choice(IDS) for _ in range(n)])
        total += n
    payload = b"".join(b"".join(varint(t) for t in s) + b"\x00" for s in sents)
    if rnd.random() < 0.5:
        payload = payload[:-1]  # (the last sentence ended by the payload)
    feats, refs = set(), {}
    for _ in range(rnd.randint(1, 10)):
        n = rnd.choice([n0, rnd.randint(3, 13)])
        fits = [i for i, s in enumerate(sents) if len(s) >= n]
        if not fits or rnd.random() < 0.25:  # an n-gram row between the skipgrams
            refs.setdefault(b"".join(varint(rnd.choice(IDS)) for _ in range(rnd.randint(1, 4))), [(rnd.randint(1, 99), rnd.randint(0, 99)) for _ in range(rnd.randint(0, 3))])
            feats.add("ngram")
            continue
        toks = [rnd.choice(IDS) for _ in range(n)]
        shape = rnd.choice(["trailing", "leading", "multi"]) if n > 3 else "single"
        gaps = [1] if shape in ("single", "trailing") else [n - 2] if shape == "leading" else sorted(rnd.sample(range(1, n - 1), rnd.randint(2, n - 2)))
        for g in gaps:
            toks[g] = 3
        feats |= {shape, "n%d" % n} | ({"n13"} if n == 13 else set())
        here = []
        for _ in range(rnd.randint(1, 5)):
            s = rnd.choice(fits)
            t = rnd.choice([0, len(sents[s]) - n, rnd.randint(0, len(sents[s]) - n)])
            feats |= {"last fitting token"} if t == len(sents[s]) - n else set()
            feats |= {"sentence of n"} if len(sents[s]) == n else set()
            feats |= {"sentence of n + 1"} if len(sents[s]) == n + 1 else set()
            window = sents[s][t:t + n]
            feats |= {"no word"} if any(w not in words for w in window) else set()
            feats |= {"empty word"} if 5 in window else set()
            feats |= {"empty first word"} if window[0] == 5 else set()
            feats |= {"multi-byte id"} if any(w >= 128 for w in window) else set()
            here.append((first + s, t))
        refs.setdefault(b"".join(varint(t) for t in toks), here)
    feats.add("first_sentence %d" % first)
    feats |= {"empty sentence"} if any(len(s) == 0 for s in sents) else set()
    feats |= {"sentence of one"} if any(len(s) == 1 for s in sents) else set()
    feats |= {"GAP"} if words[3] == b"GAP" else set()
    key_off, kb, _, r = flat(refs)
    return words, (key_off, kb, None, r), rnd.randint(1, 5000), payload, first, feats


def test_a_hundred_random_cases(ctx, monkeypatch):
    rnd = random.Random(20261)
    seen = set()
    for i in range(100):
        words, arrays, tokens, payload, first, feats = random_instance_case(rnd)
        if i % 2:
            monkeypatch.setenv("COLIBRI_PRINT_WINDOW_BYTES", str(rnd.randint(1, 9)))
            feats.add("small windows")
        else:
            monkeypatch.delenv("COLIBRI_PRINT_WINDOW_BYTES", raising=False)
        want = b"".join(instance_rows(words, arrays, tokens, payload, first))
        ctx.upload(payload, first)
        assert ctx.print_model(words, arrays, tokens, instantiate=True) == want, i
        seen |= feats | {w for w in ("[{?}", " {?}]", "  ") if w.encode() in want}
    need = {"ngram", "single", "trailing", "leading", "multi", "n3", "n13", "last fitting token", "sentence of n", "sentence of n + 1", "no word", "empty word", "empty first word",
            "multi-byte id", "first_sentence 1", "first_sentence 5", "empty sentence", "sentence of one", "GAP", "small windows"}
    assert need <= seen, need - seen


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(monkeypatch):
    from colibri_amd import capi
    words, arrays, tokens, payload = fixture_case("hamlet.v2")
    want = b"".join(instance_rows(words, arrays, tokens, payload))
    key_off, key_bytes, _, (ro, rs, rt) = arrays

    def refused(c, model, code, text):
        pieces = []
        with pytest.raises(capi.ColibriError) as e:
            c.print_model(words, model, tokens, sink=pieces.append, instantiate=True)
        assert e.value.code == code and text in str(e.value), str(e.value)
        assert pieces == []  # nothing was handed over

    with capi.Context(0) as c:
        refused(c, arrays, -6, "no corpus")  # COLIBRI_ERR_STATE
        assert c.print_model(words, arrays, tokens) == b"".join(print_rows(words, arrays, tokens))  # (the plain print needs none)
        c.upload(payload)
        assert c.print_model(words, arrays, tokens, instantiate=True) == want
        flex = (np.array([0, 3], dtype=np.uint64), np.frombuffer(b"\x06\x04\x07", dtype=np.uint8), None,
                (np.array([0, 1], dtype=np.uint64), np.array([1], dtype=np.uint32), np.array([0], dtype=np.uint16)))
        refused(c, flex, -4, "flexgrams")  # COLIBRI_ERR_UNSUPPORTED
        assert c.print_model(words, arrays, tokens, instantiate=True) == want
        # the first reference of a skipgram row moved: past its sentence's end by one token, to the sentence behind the corpus' last, to one before its first.
        # The length kernel compares numbers; nothing of such a window is read.
        from test_coverage import category_of, tokens_of
        kb = bytes(bytearray(np.asarray(key_bytes, dtype=np.uint8).tolist()))
        j = next(j for j in range(len(key_off) - 1) if category_of(tokens_of(kb[int(key_off[j]):int(key_off[j + 1])])) == 2)
        r, n = int(ro[j]), len(tokens_of(kb[int(key_off[j]):int(key_off[j + 1])]))
        from test_instantiate import sentences_of
        sent = sentences_of(payload)
        for s, t in ((int(rs[r]), len(sent[int(rs[r]) - 1]) - n + 1), (len(sent) + 1, 0), (0, 0), (2 ** 32 - 1, 65535)):
            rs2, rt2 = rs.copy(), rt.copy()
            rs2[r], rt2[r] = s, t
            refused(c, (key_off, key_bytes, None, (ro, rs2, rt2)), -1, "does not fit the corpus")  # COLIBRI_ERR_ARG
            assert c.print_model(words, arrays, tokens, instantiate=True) == want
        c.upload(payload, 1000)  # the same corpus numbered from 1000: none of the model's sentences is in it
        refused(c, arrays, -1, "does not fit the corpus")
        c.upload(payload)
        monkeypatch.setenv("COLIBRI_PRINT_BUDGET", "1")
        refused(c, arrays, -7, "COLIBRI_PRINT_BUDGET")  # COLIBRI_ERR_OVERFLOW
        monkeypatch.delenv("COLIBRI_PRINT_BUDGET")
        assert c.print_model(words, arrays, tokens, instantiate=True) == want
        unindexed = (np.array([0, 3], dtype=np.uint64), np.frombuffer(b"\x06\x03\x07", dtype=np.uint8), np.array([2], dtype=np.uint32), None)
        assert c.print_model(words, unindexed, tokens, instantiate=True) == b"".join(print_rows(words, unindexed, tokens))  # no references, no instances
