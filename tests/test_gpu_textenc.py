"""The class encoder's kernels (csrc/textenc.hpp, behind colibri_text_* in csrc/text_api.inc) through the C ABI against the plain
restatement oracle.text_words / oracle.text_encode, which tests/test_classenc.py pins to the oracle of the real reference: every
distinct word with its count and first occurrence under both sets of rules, and the encoded stream, byte for byte — at the sizes
where the kernels change path (16 bytes per thread, 4096 bytes per event block, 1024 event blocks per first-level scan block, 8-byte
word loads), with every quirk byte on every side of those boundaries, and through both collision retry loops
(COLIBRI_TEXT_HASH_BITS). All comparisons are exact.

ONE context serves the whole file, large and small texts in turn: that a context may be used again is part of what is tested."""
import zlib

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

CLASS_EDGES = [127, 128, 16383, 16384, (1 << 21) - 1, 1 << 21, (1 << 28) - 1, 1 << 28, (1 << 32) - 1]  # the ends of 1 .. 5 varint bytes
SOME_CLASSES = CLASS_EDGES + [1, 6, 300]


@pytest.fixture(scope="module")
def ctx():
    from colibri_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def some_class(w):
    return SOME_CLASSES[zlib.crc32(w) % len(SOME_CLASSES)]


def some_repeat(w):
    return 1 + (zlib.crc32(w) >> 8) % 2


def check_words(ctx, text, rules, tag=None, upload=True):
    """the shared check of the distinct words; returns them in the device's order"""
    nwords, start, length, count = ctx.text_words(text, rules) if upload else ctx.text_recount(rules)
    want = oracle.text_words(text, rules)
    words = [text[s:s + n] for s, n in zip(start.tolist(), length.tolist())]
    got = {w: [c, s] for w, c, s in zip(words, count.tolist(), start.tolist())}
    assert len(got) == len(words), (tag, rules, "the same word twice")
    assert set(got) == set(want), (tag, rules, sorted(set(got) ^ set(want))[:8])
    bad = [(w, got[w], want[w]) for w in want if got[w] != want[w]][:8]
    assert not bad, (tag, rules, "(word, [count, first_start] of the device, of the restatement)", bad)
    assert nwords == int(count.sum(dtype=np.uint64)) == sum(c for c, _ in want.values()), (tag, rules)
    assert len(start) == len(length) == len(count) == len(want), (tag, rules)  # ndistinct
    return words


def check_encode(ctx, text, words, cls=some_class, repeat=some_repeat, tag=None):
    """the shared check of the encoded stream; `words` = the distinct words in the device's order (check_words(..., 1))"""
    cls_of = {w: cls(w) for w in words}
    rep_of = {w: repeat(w) for w in words}
    got = ctx.text_encode(np.array([cls_of[w] for w in words], dtype=np.uint32), np.array([rep_of[w] for w in words], dtype=np.uint32))
    want = oracle.text_encode(text, cls_of, rep_of)
    assert got[1:] == want[1:], (tag, "(ntokens, nlines)")
    assert got[0] == want[0], (tag, len(got[0]), len(want[0]), next((k for k, (a, b) in enumerate(zip(got[0], want[0])) if a != b), None))
    return got


def check_text(ctx, text, tag=None):
    check_words(ctx, text, 0, tag)
    words = check_words(ctx, text, 1, tag)
    return check_encode(ctx, text, words, tag=tag)


# every event kind: a segment start, a newline, a run of spaces, \t and \r as no-words, \b and \t\r trims, \r\n, a \t and a \r before a
# line-final space (the frequency list's empty word), a multi-byte character, no final newline
QUIRK = b"ab \t \r\n\t\r x\b\t  {*} \xc3\xa9\n\t \nq y\b \r \nzz\t\b\r w"
assert len(QUIRK) == 40

ALPHABET = [b"a", b"b", b"ab", b"the", b"cat", b"\t", b"\r", b"x\t", b"\tx", b"{*}", b"{**}", b"{?}", b"{*2*}", b"\b", b"y\b", "é".encode(), b"zz" * 120,
            b"\t\r", b"\r", b"\b", b"x\b\t"]


def quirk_text(rng, nlines):
    """test_classenc.random_text's grammar and words, plus \\t\\r, \\b, x\\b\\t, \\r\\n line ends and \\t / \\r before a line-final space"""
    out = []
    for _ in range(nlines):
        n = int(rng.integers(0, 12))
        head = np.minimum(rng.pareto(0.8, size=n).astype(np.int64), len(ALPHABET) - 1)
        idx = np.where(rng.random(n) < 0.5, head, rng.integers(0, len(ALPHABET), size=n))
        line = b"".join(ALPHABET[int(i)] + b" " * int(rng.integers(1, 3)) for i in idx)
        r = rng.random()
        if r < 0.15:
            line += b"\t "
        elif r < 0.3:
            line += b"\r "
        elif r < 0.5:
            line = line.rstrip(b" ")
        out.append(line + (b"\r\n" if rng.random() < 0.2 else b"\n"))
    text = b"".join(out)
    return text if rng.random() < 0.7 else text[:-1].rstrip(b"\r")


# ---- thread (16 bytes) and event block (4096 bytes) boundaries ---------------------------------------------------------------------
@pytest.mark.parametrize("lo", [0, 4080])
def test_every_event_kind_at_every_offset_round_a_boundary(ctx, lo):
    filler = b"fill " * 900
    for p in range(lo, lo + 34):
        for tail in (b"", b"\n"):
            check_text(ctx, filler[:p] + QUIRK + tail, tag=(p, tail))


# ---- counting: block-local election and `first`, the table at its design load (large texts between the small ones) ------------------
def lines_of(words, per_line=23):
    return b"".join(b" ".join(words[k:k + per_line]) + b"\n" for k in range(0, len(words), per_line))


def test_one_hot_word_and_rare_words_first_seen_in_the_last_1024_events(ctx):
    words = [b"hot"] * 300_000
    for k, rare in enumerate([b"r1", b"rare2", b"r3\t", b"\tr4", b"r5"]):
        words[-900 + 170 * k] = rare  # 300 000 words + 13 044 newlines: all of these lie in the last 1024 events
        words[-890 + 170 * k] = rare
    check_text(ctx, lines_of(words), "hot+rare")


# ---- the 8-byte word walk: text_word_of_segment, text_hash and the masked tail compare of text_verify_kernel -----------------------
WORD_LENGTHS = list(range(1, 34)) + [63, 64, 65, 255, 256, 4095, 4096, 4097, 70_000]
ANY = np.array([b for b in range(256) if b not in (0x20, 0x0A)], dtype=np.uint8)
FIRM = np.array([b for b in ANY if b not in (9, 13, 8)], dtype=np.uint8)  # not trimmed under either set of rules


def word_and_twins(rng, n):
    """a word of n bytes, one that differs only in its last byte, one that is one byte shorter (none of them ends in a trimmed byte)"""
    w = ANY[rng.integers(0, ANY.size, size=n)]
    w[-2:] = FIRM[rng.integers(0, FIRM.size, size=min(2, n))]
    last = FIRM[FIRM != w[-1]][int(rng.integers(0, FIRM.size - 1))]
    w = w.tobytes()
    return [w, w[:-1] + bytes([int(last)]), w[:-1]]


def test_words_of_every_length_with_twins_and_at_the_end_of_the_text(ctx):
    rng = np.random.default_rng(31)
    small = []
    for n in WORD_LENGTHS:
        w, t1, t2 = word_and_twins(rng, n)
        if n <= 256:
            small += [w, t1, t2]
        for last in (w, t1, t2):
            # (t2 of a one-byte word is empty: two separators in a row)
            check_text(ctx, w + b" " + t1 + b"\n" + t2 + b" " + w + b" " + last, tag=(n, len(last)))
    rng.shuffle(small)
    check_text(ctx, lines_of(small * 3, 5)[:-1], "all lengths in one text")


def test_trim_tails_across_an_eight_byte_load(ctx):
    rng = np.random.default_rng(32)
    tails = [b""] + [bytes(rng.choice([9, 13, 8], size=k).tolist()) for k in range(1, 10) for _ in range(3)] + [bytes([c]) * k for c in (9, 13, 8) for k in (1, 7, 8, 9)]
    toks = [b"abcdefghi"[:k] + t for k in range(0, 10) for t in tails]  # k = 0: a segment of trimmed bytes alone
    order = rng.permutation(len(toks))
    text = lines_of([toks[int(i)] for i in order], 7)
    check_text(ctx, text, "tails")
    for last in (b"abcdefg\t", b"abcdefgh\b", b"abcdefgh\t\r\b\b\t", b"\t\r", b"\b", b"a\b\b\b\b\b\b\b\b\b"):
        check_text(ctx, text + last, ("tails", last))
    # the same word or two words, by the rules
    w0 = check_words(ctx, b"ab ab\t ab\b ab\r ab\b\t ab\t\b\nab\b ab", 0)
    w1 = check_words(ctx, b"ab ab\t ab\b ab\r ab\b\t ab\t\b\nab\b ab", 1)
    assert sorted(w0) == [b"ab", b"ab\b", b"ab\t\b"] and w1 == [b"ab"]


def test_two_hot_words_alternating(ctx):
    check_text(ctx, lines_of([b"aa", b"bb"] * 150_000), "two hot")


# ---- the grammar at random ---------------------------------------------------------------------------------------------------------
def test_200_random_quirk_texts(ctx):
    rng = np.random.default_rng(33)
    for k in range(200):
        check_text(ctx, quirk_text(rng, int(rng.integers(1, 40)))[:2048], k)


@pytest.mark.parametrize("n", [1, 15, 16, 17, 4095, 4096, 4097])
def test_texts_of_exactly_n_bytes(ctx, n):
    rng = np.random.default_rng(34)
    random = b"".join(quirk_text(rng, 40) for _ in range(12))
    assert len(random) >= 4097 + 5
    for k, text in enumerate([b"a" * n, b" " * n, b"\n" * n, b"\t" * n, b"a " * n, b"a\n" * n, b" a" * n, QUIRK * 110, QUIRK[7:] * 130, random, random[5:]]):
        check_text(ctx, text[:n], (n, k))


def test_200_000_distinct_words_fill_the_table_to_its_design_load(ctx):
    check_text(ctx, lines_of([b"w%x" % k for k in range(200_000)]), "distinct")  # cap = 1.5 n + 1024


# ---- the encoder's edges -----------------------------------------------------------------------------------------------------------
def test_encode_class_ids_at_the_varint_edges_and_repeats(ctx):
    pairs = [(c, r) for c in CLASS_EDGES for r in (0, 1, 2, 300)]
    table = {b"w%d" % k: p for k, p in enumerate(pairs)}
    rng = np.random.default_rng(35)
    names = list(table)
    text = lines_of([names[int(i)] for i in rng.integers(0, len(names), size=700)], 9)
    words = check_words(ctx, text, 1)
    assert set(words) == set(names)
    payload, ntokens, nlines = check_encode(ctx, text, words, cls=lambda w: table[w][0], repeat=lambda w: table[w][1])
    assert nlines == 78 and ntokens == sum(table[w][1] for w in text.split())
    # two encodes with different maps after one count: the second is right too
    check_encode(ctx, text, words, cls=lambda w: table[w][0] ^ 5, repeat=lambda w: (table[w][1] + 1) % 4)
    check_encode(ctx, text, words)


def test_encode_drops_what_follows_the_last_newline_by_itself(ctx):
    one = lambda w: 1
    text = b"a b\nb c\nonlyafter b"  # `onlyafter` has no occurrence before the last newline, `b` has them on both sides
    words = check_words(ctx, text, 1)
    assert sorted(words) == [b"a", b"b", b"c", b"onlyafter"]
    payload, ntokens, nlines = check_encode(ctx, text, words, cls=lambda w: {b"a": 6, b"b": 7, b"c": 8, b"onlyafter": 9}[w], repeat=one)
    assert (payload, ntokens, nlines) == (bytes([6, 7, 0, 7, 8, 0]), 4, 2)
    for text in (b"no newline at all", b"x", b"a  b \t c\r"):
        assert check_encode(ctx, text, check_words(ctx, text, 1), repeat=one) == (b"", 0, 0)
    assert check_words(ctx, b"", 0) == [] and check_words(ctx, b"", 1) == []
    assert check_encode(ctx, b"", []) == (b"", 0, 0)
    for text, nl in ((b" \n\n  \n ", 3), (b"\n", 1), (b"   ", 0), (b"\t \r \n \t\r\n\r\n", 3)):
        assert check_words(ctx, text, 1) == []
        assert check_encode(ctx, text, []) == (b"\0" * nl, 0, nl)
        check_words(ctx, text, 0)


def test_zipf_text_of_300_000_words(ctx):
    rng = np.random.default_rng(36)
    vocab = 40_000
    p = 1.0 / np.arange(1, vocab + 1)
    ranks = np.searchsorted(np.cumsum(p / p.sum()), rng.random(300_000))
    names = [b"z%x" % k for k in range(vocab)]
    check_text(ctx, lines_of([names[int(r)] for r in ranks], 17), "zipf")


# ---- call order and refusals -------------------------------------------------------------------------------------------------------
def test_call_order_and_refusals_leave_a_working_context(ctx):
    import ctypes as C
    from colibri_amd import capi
    L, h = ctx.L, ctx.h
    text = b"one two\none"
    a, b, c = (np.zeros(8, dtype=np.uint32) for _ in range(3))
    ptr = lambda x: x.ctypes.data
    o = [C.c_uint64() for _ in range(3)]
    assert L.colibri_text_upload(h, text, len(text)) == capi.OK
    assert L.colibri_text_words(h, ptr(a), ptr(b), ptr(c)) == capi.ERR_STATE  # no count yet
    assert L.colibri_text_encode(h, ptr(a), ptr(b), C.byref(o[0]), C.byref(o[1]), C.byref(o[2])) == capi.ERR_STATE
    assert L.colibri_text_fetch(h, ptr(a)) == capi.ERR_STATE
    assert L.colibri_text_count(h, 2, C.byref(o[0]), C.byref(o[1])) == capi.ERR_ARG
    assert L.colibri_text_count(h, -1, C.byref(o[0]), C.byref(o[1])) == capi.ERR_ARG
    assert L.colibri_text_count(h, 0, C.byref(o[0]), C.byref(o[1])) == capi.OK and (o[0].value, o[1].value) == (3, 2)
    assert L.colibri_text_encode(h, ptr(a), ptr(b), C.byref(o[0]), C.byref(o[1]), C.byref(o[2])) == capi.ERR_STATE  # the frequency list's rules
    assert ctx.text_recount(0)[0] == 3
    with pytest.raises(capi.ColibriError) as e:
        ctx.text_encode(a[:2], b[:2])
    assert e.value.code == capi.ERR_STATE
    with pytest.raises(capi.ColibriError) as e:
        ctx.text_recount(2)
    assert e.value.code == capi.ERR_ARG
    # 2 GiB announced over an 11-byte buffer: refused before any byte is read
    assert L.colibri_text_upload(h, text, 0x7FFFFFF0) == capi.ERR_CORPUS
    with pytest.raises(capi.ColibriError) as e:
        ctx._check(L.colibri_text_upload(h, text, 0x7FFFFFF0))
    assert e.value.code == capi.ERR_CORPUS and "2 GiB" in str(e.value)
    check_text(ctx, text, "after the refusals")


# ---- the second level of the event scan: more than 1024 event blocks of 4096 bytes ---------------------------------------------------
def test_text_just_over_4_MiB_reaches_the_second_scan_level(ctx):
    rng = np.random.default_rng(37)
    n = 4 * (1 << 20) + 4097
    alphabet = np.array(ALPHABET + [b"w%d" % k for k in range(40)], dtype=object)
    weight = np.ones(alphabet.size)
    weight[ALPHABET.index(b"zz" * 120)] = 3.0  # long words keep the word count, and so the restatement's time, down
    seps = np.array([b" ", b"  ", b"\n", b"\r\n", b" \n", b"\t \n", b"\r \n"], dtype=object)
    m = 400_000
    toks = alphabet[rng.choice(alphabet.size, size=m, p=weight / weight.sum())]
    gaps = seps[rng.choice(seps.size, size=m, p=[0.6, 0.1, 0.1, 0.05, 0.05, 0.05, 0.05])]
    text = b"".join(np.stack([toks, gaps], axis=1).ravel().tolist())
    assert len(text) >= n
    check_text(ctx, text[:n], "4 MiB")
    check_text(ctx, QUIRK, "small after large")


# ---- the collision retry loop of colibri_text_count, forced by COLIBRI_TEXT_HASH_BITS ----------------------------------------------
def hook_text():
    return b"".join(quirk_text(np.random.default_rng(38), 40) for _ in range(6))  # ~1500 words, far below 10 000: every key lands in two slots


@pytest.mark.parametrize("attempts", [1, 2, 3])
def test_collisions_in_the_first_attempts_are_retried_under_another_seed(ctx, monkeypatch, attempts):
    from colibri_amd import capi, synth
    text = hook_text()
    assert min(len(oracle.text_words(text, r)) for r in (0, 1)) >= 3  # one bit of hash: two of three words collide
    # a profiled run of the trainer switches the context's kernel events on: every attempt of a count is then one launch of COLIBRI_K_COUNT
    ctx.upload(synth.zipf_corpus(2000, 50, 7, header=False))
    ctx.train(mintokens=2, maxlength=2, profile=1)
    attempts_run = lambda: ctx.kernel_time(capi.K_COUNT)[1]
    plain = {}
    for rules in (0, 1):
        before = attempts_run()
        nwords, start, length, count = ctx.text_words(text, rules)
        assert attempts_run() - before == 1
        plain[rules] = (nwords, {text[s:s + n]: (c, s) for s, n, c in zip(start.tolist(), length.tolist(), count.tolist())})
    words = check_words(ctx, text, 1, upload=False)
    plain_encoded = check_encode(ctx, text, words)
    monkeypatch.setenv("COLIBRI_TEXT_HASH_BITS", f"1:{attempts}")
    for rules in (0, 1):
        before = attempts_run()
        nwords, start, length, count = ctx.text_words(text, rules)
        assert attempts_run() - before == attempts + 1, "every masked attempt collides and is retried; the first unmasked one succeeds"
        assert (nwords, {text[s:s + n]: (c, s) for s, n, c in zip(start.tolist(), length.tolist(), count.tolist())}) == plain[rules]
        words = check_words(ctx, text, rules, ("hooked", attempts), upload=False)
    assert check_encode(ctx, text, words, tag=("hooked", attempts)) == plain_encoded


@pytest.mark.parametrize("setting", ["1", "1:4"])
def test_four_collisions_are_refused_and_leave_no_count_behind(ctx, monkeypatch, setting):
    import ctypes as C
    from colibri_amd import capi
    text = hook_text()
    for rules in (0, 1):
        words = check_words(ctx, text, 1)  # a count that succeeded: the state a failing one must not leave readable
        monkeypatch.setenv("COLIBRI_TEXT_HASH_BITS", setting)
        with pytest.raises(capi.ColibriError) as e:
            ctx.text_recount(rules)
        assert "four" in str(e.value) and "seeds" in str(e.value)
        a, b, c = (np.ones(len(words) + 1, dtype=np.uint32) for _ in range(3))
        assert ctx.L.colibri_text_words(ctx.h, a.ctypes.data, b.ctypes.data, c.ctypes.data) == capi.ERR_STATE
        with pytest.raises(capi.ColibriError) as e:
            ctx.text_encode(a, b)
        assert e.value.code == capi.ERR_STATE
        assert ctx.L.colibri_text_fetch(ctx.h, a.ctypes.data) == capi.ERR_STATE
        monkeypatch.delenv("COLIBRI_TEXT_HASH_BITS")
        check_words(ctx, text, 0, "after the refusal", upload=False)
        check_encode(ctx, text, check_words(ctx, text, 1, "after the refusal", upload=False))
