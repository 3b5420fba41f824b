"""Expanding a loaded model on further corpus data on the device (colibri_set_seed + colibri_train + colibri_seed_fetch; csrc/expand.hpp): through the C ABI
against the plain restatement (tests/expand_models.py, which tests/test_expand.py pins to the real reference), and through the C++ face and the CLI
(colibri-patternmodeller -i m -f corpus -e N without -E) against the reference's own results (tests/golden/expand/)."""
import functools
import os
import subprocess

import numpy as np
import pytest

import expand_models as em
from colibri_amd import capi, synth
from conftest import GOLDEN, ROOT
from test_expand import CASES, golden, payload
from test_host_face import CLI, parse_model

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def corpus(vocab, seed):
    """~3000 tokens; vocab 100: every token one byte (classes 6 .. 105), vocab 400: one- and two-byte tokens, so keys of one length in tokens differ in bytes"""
    return synth.zipf_corpus(3000, vocab, seed, header=False)


@functools.lru_cache(maxsize=None)
def seed_model(vocab, t, l, indexed):
    return em.train(corpus(vocab, 11), t, l, indexed=indexed)


def device_expand(seed, data, t, l, indexed=False, first=1):
    with capi.Context(0) as ctx:
        ctx.upload(data, first_sentence=first)
        got, st = ctx.expand_dict(seed, mintokens=t, maxlength=l, indexed=int(indexed))
    return got, st


def check(seed, data, t, l, indexed=False, first=1):
    """the device's merged model and figures against the restatement's; returns both"""
    want = em.expand(seed, data, t, l, indexed=indexed, firstsentence=first)
    got, st = device_expand(seed, data, t, l, indexed, first)
    if indexed:
        assert got == want.refs  # (every list ascending, duplicates kept: IndexedPatternModel::posttrain)
    else:
        assert got == want.counts
    assert st.totaltokens == want.tokens
    assert st.maxn == want.maxn
    stop = want.stop if want.stop else 0
    last = stop if stop else min(l, max(want.found) if want.found else 0)
    assert [st.found[n] for n in range(1, last + 1)] == [want.found[n] for n in range(1, last + 1)]
    if seed:  # what each order's prune erased, never-seen loaded patterns included; nothing at the order the run stopped at or beyond the last one visited
        assert [st.pruned[n] for n in range(1, l + 2)] == [want.pruned.get(n, 0) for n in range(1, l + 2)]
        assert all(st.kept[n] + st.pruned[n] >= st.found[n] for n in range(1, l + 1))
    if seed and want.maxn >= 1:
        assert st.totaltypes == want.types
    if seed:
        assert st.path == capi.PATH_TABLE | capi.PATH_PER_PASS | (st.path & (capi.PATH_PAIRS_WHOLE | capi.PATH_PAIRS_UNPACKED))
    return want, got, st


@pytest.mark.parametrize("first", [1, 1000])
@pytest.mark.parametrize("indexed", [False, True])
@pytest.mark.parametrize("l", [1, 2, 5])
@pytest.mark.parametrize("t", [2, 3])
@pytest.mark.parametrize("vocab", [100, 400])
def test_expand_matches_the_restatement(vocab, t, l, indexed, first):
    """a model of one Zipf corpus expanded on another: class spaces on both sides of 128, so the join compares keys of one- and two-byte tokens"""
    m = seed_model(vocab, t, l, indexed)
    want, _, _ = check(m.refs if indexed else m.counts, corpus(vocab, 12), t, l, indexed, first)
    if l > 1:
        naive = em.naive_sum(m.counts, em.train(corpus(vocab, 12), t, l).counts)
        assert any(naive.get(k) != c for k, c in want.counts.items())  # (a run that added two separate models would not pass)


def test_an_empty_seed_set_is_a_plain_train():
    import oracle
    data = corpus(400, 12)
    want = oracle.train(data, 2, 5)
    got, st = device_expand({}, data, 2, 5)
    assert got == want.counts and (st.totaltokens, st.totaltypes) == (want.tokens, want.types)


def key(*classes):
    return synth.encode_v2(np.array(classes, dtype=np.uint32)).tobytes()


def sents(*sentences):
    return b"".join(key(*s) + b"\x00" for s in sentences)


A, B, C, D, X, P, Q, R, S, U, V, W = 6, 7, 200, 9, 300, 11, 12, 13, 14, 500, 16, 17  # (C, X, U: two-byte tokens)


def test_seeds_that_are_not_closed_under_subwindows():
    """the seeds lack their sub-windows and carry count 1: "a b c d" occurs once and survives only as 1 + 1; its window is counted although "a b" was pruned
    at order 2, because "a b c" — never counted here — is a loaded pattern that stays (the look-back asks the model as it stands). A seed at t - 1 in total is
    pruned though loaded; seeds the corpus never contains go or stay by their own count at a pruned order, and stay above the last order"""
    data = sents((A, B, C, D), (X, B, C, D), (P, Q, R, S), (P, Q, R, S), (V, W), (W,), (V,))
    seed = {key(A, B, C): 5, key(A, B, C, D): 1, key(V, W): 0, key(U, V): 1, key(U, W): 3, key(U, U, U, U, U, U): 1, key(Q, R): 1}
    want, got, st = check(seed, data, 2, 4)
    assert got[key(A, B, C, D)] == 2 and got[key(A, B, C)] == 5 and key(A, B) not in got
    assert key(V, W) not in got and key(U, V) not in got and got[key(U, W)] == 3 and got[key(U, U, U, U, U, U)] == 1 and got[key(Q, R)] == 3
    assert want.stop == 0 and st.maxn == 4
    with capi.Context(0) as ctx:  # the same run, the seeds' rows looked at directly
        ctx.upload(data)
        keys = list(seed)
        ctx.set_seed(keys, [seed[k] for k in keys])
        ctx.train(mintokens=2, maxlength=4)
        row, kept = ctx.seed_state()
        cd, _ = ctx.export_dict()
        key_off, key_bytes, counts, _ = ctx.export_arrays()
    rows = {k: (int(r), int(f)) for k, r, f in zip(keys, row, kept)}
    assert [rows[k][1] for k in keys] == [1, 1, 0, 0, 1, 1, 1]
    assert rows[key(A, B, C)][0] == capi.NO_PATTERN and rows[key(U, W)][0] == capi.NO_PATTERN and rows[key(V, W)][0] == capi.NO_PATTERN
    kb = key_bytes.tobytes()
    for k in (key(A, B, C, D), key(Q, R)):
        r = rows[k][0]
        assert kb[int(key_off[r]): int(key_off[r + 1])] == k and int(counts[r]) == cd[k]


def test_a_corpus_that_creates_no_unigram_stops_at_order_1():
    """every token of the corpus is a loaded unigram: the run stops at order 1 before the prune — the sums stay though below the threshold, maxn and the type
    count are untouched, no bigram is counted"""
    data = sents((A, B, A), (D,))
    seed = {key(A): 1, key(B): 1, key(D): 1, key(A, B): 1, key(U, U, U): 1}  # (the last: never in the corpus, above the stop order, below the threshold: it stays)
    want, got, st = check(seed, data, 5, 3)
    assert want.stop == 1 and st.maxn == 0 and st.totaltypes == 0 and st.found[1] == 0 and st.pruned[1] == 0
    assert got == {key(A): 3, key(B): 2, key(D): 2, key(A, B): 1, key(U, U, U): 1}


@pytest.mark.parametrize("indexed", [False, True])
def test_the_seeds_own_corpus_stops_at_a_middle_order(indexed):
    """a model expanded on the corpus it came from creates the pruned patterns of the low orders again and nothing at order 4: that order's rows leave unpruned,
    with doubled counts, and the loaded 5-grams keep theirs"""
    m = em.train(payload("hamlet.v2"), 2, 5, indexed=indexed)
    seed = dict(m.refs if indexed else m.counts)
    unseen = key(3000000, 3000001, 3000000, 3000001, 3000000)  # a loaded 5-gram the corpus never contains, with count 1: above the stop order it stays
    seed[unseen] = [(7, 0)] if indexed else 1
    want, got, st = check(seed, payload("hamlet.v2"), 2, 5, indexed, first=1)
    assert (got[unseen] == [(7, 0)] if indexed else got[unseen] == 1) and st.pruned[4] == 0 and st.pruned[5] == 0
    assert want.stop == 4 and st.maxn == 3 and st.found[4] == 0 and st.kept[4] > 0
    four = [k for k in m.counts if em.ntokens(k) == 4]
    assert four and all(len(got[k]) == 2 * m.counts[k] if indexed else got[k] == 2 * m.counts[k] for k in four)


def test_sentences_shorter_than_the_order():
    """no sentence has three tokens: order 3 counts nothing, creates nothing and stops; the loaded trigram stays"""
    data = sents((A, B), (A, B), (D,), (A, B), (), (D, A))
    want, got, st = check({key(A, B, D): 1, key(A): 1}, data, 2, 5)
    assert want.stop == 3 and st.maxn == 2 and got[key(A, B, D)] == 1 and got[key(A, B)] == 3 and got[key(A)] == 5


@pytest.mark.parametrize("indexed", [False, True])
def test_a_corpus_with_empty_sentences(indexed):
    """tests/golden/edge.colibri.dat has empty sentences: they take a sentence number and nothing else"""
    m = em.train(payload("shortlines"), 2, 4, indexed=indexed)
    check(m.refs if indexed else m.counts, payload("edge"), 2, 4, indexed, first=1000)


def test_what_a_seeded_run_refuses():
    with capi.Context(0) as ctx:
        ctx.upload(corpus(100, 12))
        with pytest.raises(capi.ColibriError) as e:
            ctx.set_seed([key(A, 3, B)], [2])  # 03: the skip class
        assert e.value.code == capi.ERR_UNSUPPORTED and "skipgrams and flexgrams" in str(e.value)
        with pytest.raises(capi.ColibriError) as e:
            ctx.set_seed([key(A), key(4)], [2, 2])  # 04: the flex class
        assert e.value.code == capi.ERR_UNSUPPORTED
        ctx.set_seed([key(A)], [2])
        with pytest.raises(capi.ColibriError) as e:
            ctx.seed_state()
        assert e.value.code == capi.ERR_STATE
        for kw in (dict(mintokens=1), dict(minlength=2), dict(indexed=1, doskipgrams=1), dict(doskipgrams_exhaustive=1), dict(maxbackofflength=2), dict(mintokens_unigrams=4),
                   dict(dopatternperline=1)):
            with pytest.raises(capi.ColibriError) as e:
                ctx.train(**{"mintokens": 2, "maxlength": 5, **kw})
            assert e.value.code == capi.ERR_UNSUPPORTED and "expanding a loaded model" in str(e.value), kw
        rc = ctx.L.colibri_set_seed(ctx.h, None, None, None, 2 ** 31 - 16)  # the seed limit: a seed's number must fit beside the flag of a look-back id
        assert rc == capi.ERR_OVERFLOW and b"seed set too large" in ctx.L.colibri_last_error(ctx.h)
        ctx.set_seed([key(A)], [0xFFFFFFFF])  # a loaded count plus the corpus' must fit 32 bits
        with pytest.raises(capi.ColibriError) as e:
            ctx.train(mintokens=2, maxlength=2)
        assert e.value.code == capi.ERR_OVERFLOW and "exceeds 2^32 - 1" in str(e.value)
        ctx.set_constraint([key(A)])  # another set ends the mode: an ordinary constrained run
        assert ctx.train(mintokens=1, maxlength=2).npatterns == 1
        ctx.set_seed([key(A)], [2])
        ctx.set_seed([], [])  # ... and so does an empty one
        assert ctx.train(mintokens=1, maxlength=1).npatterns > 1


# ---- the C++ face and the CLI against the reference's results ----------------------------------------------------------------------------------------------------
def cli(*args):
    return subprocess.run([CLI] + [str(a) for a in args], capture_output=True, text=True)


@pytest.mark.parametrize("tag", list(CASES))
def test_cli_expand_matches_the_reference(tmp_path, tag):
    """colibri-patternmodeller -f c1 -o m; then -i m -f c2 -e N -o m2 (and once more for the chains): the model file the reference writes after the same steps"""
    first, more, l, t, indexed = CASES[tag]
    flags = ["-l", l, "-t", t] + ([] if indexed else ["-u"])
    model = tmp_path / "m0.colibri.patternmodel"
    out = cli("-f", os.path.join(GOLDEN, first + ".colibri.dat"), "-o", model, *flags)
    assert out.returncode == 0, out.stderr
    for step, (name, fs) in enumerate(more, 1):
        nxt = tmp_path / f"m{step}.colibri.patternmodel"
        out = cli("-i", model, "-f", os.path.join(GOLDEN, name + ".colibri.dat"), "-e", fs, "-o", nxt, *flags)
        assert out.returncode == 0, out.stderr
        assert "Expanding model on" in out.stderr
        model = nxt
    head, counts, refs = golden(tag)
    mtype, tokens, types, got, gotrefs = parse_model(str(model))
    assert (mtype, tokens, types) == (20 if indexed else 10, head["tokens"], head["types"])
    assert got == counts
    if indexed:
        assert gotrefs == refs


@pytest.mark.parametrize("flag,name", [(["-s"], "-s"), (["-L"], "-L"), (["-I"], "-I"), (["-F", "S"], "-F"), (["--gpus", "2"], "--gpus"), (["-j", "MODEL"], "-j")])
def test_cli_expand_refuses_what_it_cannot_combine(tmp_path, flag, name):
    model = tmp_path / "m.colibri.patternmodel"
    data = os.path.join(GOLDEN, "hamlet.v2.colibri.dat")
    assert cli("-f", data, "-o", model, "-l", 3, "-u").returncode == 0
    out = cli("-i", model, "-f", data, "-e", 1000, "-u", "-l", 3, *[str(model) if f == "MODEL" else f for f in flag])
    assert out.returncode == 2 and f"-e without -E (expanding the loaded model on different corpus data) can not be combined with {name}" in out.stderr, out.stderr


def test_the_join_has_its_own_kernel_class():
    """a profiled seeded run books the seed join under K_JOIN (DESIGN.md 5l's figures are that clock's); an unseeded run books nothing there"""
    m = seed_model(400, 2, 5, False)
    keys = list(m.counts)
    with capi.Context(0) as ctx:
        ctx.upload(corpus(400, 12))
        ctx.train(mintokens=2, maxlength=5, table_mode=1, profile=1)
        assert ctx.kernel_time(capi.K_JOIN)[1] == 0
        ctx.set_seed(keys, [m.counts[k] for k in keys])
        st = ctx.train(mintokens=2, maxlength=5, profile=1)
        ms, launches = ctx.kernel_time(capi.K_JOIN)
        assert ms > 0 and launches >= st.maxn and capi.KERNEL_CLASSES[capi.K_JOIN] == "join"
