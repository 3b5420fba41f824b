"""The forward index's three reference forms, and token offsets that wrap at 65 536, against the oracle — every list in its order.

An indexed model's references (sentence, token) travel to the sort that groups them by pattern in one of three layouts, chosen per upload from the number of
sentences (sb bits for nsent + 2) and the longest sentence (tb bits, at most 16) — csrc/colibri_hip.hip pairs_begin / colibri_train_once:
  split      sb + tb <= 32   two u32 arrays; isort_*, the hot unigrams' bypass (emit_hot_*), direct pairs
  whole      sb + tb == 33   one u64 id << 33 | sentence << tb | token; sort64_*
  unpacked   sb + tb  > 33   id << 32 | position; the look-up in the last sort64 pass
colibri_stats.path says which one ran (COLIBRI_PATH_PAIRS_WHOLE / _UNPACKED; neither: split) and every test here asserts it.

The reference keeps the token offset as uint16_t (include/datatypes.h) and sorts every list in posttrain (include/patternmodel.h:2703): in a corpus with a
sentence of more than 65 536 tokens a pattern's list is ordered by (sentence, token mod 65536), which is not corpus order. Such corpora keep whole pairs and sort
them by the whole word; where the pairs would have to carry positions (more than 131 070 sentences as well) the run is refused.

Reference: oracle.train (pinned to the real reference for exactly such a corpus by tests/test_oracle.py::test_oracle_orders_wrapped_token_offsets_as_the_reference).
All comparisons are exact."""
import functools
import subprocess

import numpy as np
import pytest

from conftest import small_corpora

pytestmark = pytest.mark.gpu


# ---- the corpus ------------------------------------------------------------------------------------------------------------------------------------------------
def forms_corpus(nsent, longs, seed=7001):
    """`nsent` sentences in all, as the library counts them: short ones of 1-3 tokens (one in ~500 empty), the sentences of `longs` tokens spread evenly among them, the
    last one without its end marker. Classes: ~300 Zipf-distributed ones from 6 up (more than 256 survive a threshold of 2: the first 256 survivors are the hot
    unigrams, the others go through the sort) and 60 from 9000 up (never hot). A long sentence that reaches token 65 540 holds the same word at tokens 65 534-65 539,
    so windows of every order start on both sides of the wrap. Returns a v2 payload without header."""
    from colibri_amd import synth
    rng = np.random.default_rng([seed, nsent] + list(longs))
    nshort = nsent - len(longs)
    lens = rng.integers(1, 4, size=nshort)
    lens[rng.random(nshort) < 0.002] = 0
    lens[-1] = 2  # (the unterminated last sentence must hold a token to be one)
    at = [(k + 1) * nshort // (len(longs) + 1) for k in range(len(longs))]
    lens = np.insert(lens, at, longs)
    starts = np.concatenate([[0], np.cumsum(lens)])
    ntok = int(starts[-1])
    toks = 6 + np.floor(rng.pareto(0.8, size=ntok)).astype(np.int64) % 300
    high = rng.random(ntok) < 0.08
    toks[high] = 9000 + rng.integers(0, 60, size=int(high.sum()))
    for j, (a, L) in enumerate(zip(at, longs)):
        s = int(starts[a + j])  # (np.insert counts `at` in the array before the insertion)
        assert int(lens[a + j]) == L
        if L >= 65540:
            toks[s + 65534: s + 65540] = 6
    sym = np.insert(toks.astype(np.uint32), starts[1:-1], np.uint32(0))
    return synth.encode_v2(sym).tobytes()


@functools.lru_cache(maxsize=None)
def corpus(nsent, *longs):
    return forms_corpus(nsent, longs)


def sentence_count(payload):
    """sentences as colibri_upload_corpus counts them: end markers, plus a last sentence without one"""
    return payload.count(0) + (1 if payload and payload[-1] != 0 else 0)


KINDS = {
    "indexed": dict(indexed=1, maxlength=3),
    "skipgrams": dict(indexed=1, doskipgrams=1, maxlength=4),
    "order1_class": dict(indexed=1, firstsentence=77, maxlength=1),  # (order 1 alone is emitted in class form)
    "thr3": dict(indexed=1, maxlength=3, mintokens=3),
}
SPLIT, WHOLE, UNPACKED = "split", "whole", "unpacked"


def form_of(st):
    from colibri_amd import capi
    whole, unpacked = bool(st.path & capi.PATH_PAIRS_WHOLE), bool(st.path & capi.PATH_PAIRS_UNPACKED)
    assert not (whole and unpacked), st.path
    return WHOLE if whole else UNPACKED if unpacked else SPLIT


@pytest.fixture(scope="module")
def ctx():
    from colibri_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=2)
def _oracle(payload, items):
    import oracle
    kw = dict(items)
    return oracle.train(payload, kw.pop("mintokens", 2), kw.pop("maxlength"), **{k: (bool(v) if k in ("indexed", "doskipgrams") else v) for k, v in kw.items()})


def compare_lists(got, gotrefs, want, what=""):
    """patterns and counts; every list's references as a multiset; every list's order — each with its own message"""
    assert got == want.counts, f"{what}: pattern set / counts differ from the oracle ({len(got)} patterns against {len(want.counts)})"
    assert gotrefs.keys() == want.refs.keys(), what
    wrong = [k for k, r in want.refs.items() if len(gotrefs[k]) != len(r) or sorted(gotrefs[k]) != sorted(r)]
    assert not wrong, (f"{what}: {len(wrong)} of {len(want.refs)} lists hold the WRONG REFERENCES, e.g. {wrong[0].hex()}: "
                       f"{gotrefs[wrong[0]][:6]} ... against {want.refs[wrong[0]][:6]} ...")
    wrong = [k for k, r in want.refs.items() if gotrefs[k] != r]
    if wrong:
        k = wrong[0]
        j = next(i for i, (a, b) in enumerate(zip(gotrefs[k], want.refs[k])) if a != b)
        pytest.fail(f"{what}: {len(wrong)} of {len(want.refs)} lists hold the right references in the WRONG ORDER, e.g. {k.hex()} from entry {j}: "
                    f"{gotrefs[k][j:j + 4]} against {want.refs[k][j:j + 4]}")


def compare(ctx, payload, kind, what=""):
    """one train() against the oracle; returns the statistics"""
    kw = dict(kind)
    want = _oracle(payload, tuple(sorted(kw.items())))
    firstsentence, maxlength = kw.pop("firstsentence", 1), kw.pop("maxlength")
    ctx.upload(payload, first_sentence=firstsentence)
    st = ctx.train(maxlength=maxlength, **{"mintokens": 2, **kw})
    got, gotrefs = ctx.export_dict()
    compare_lists(got, gotrefs, want, what)
    assert st.nrefs == sum(len(r) for r in want.refs.values()), what
    assert (st.totaltokens, st.totaltypes, st.npatterns, st.maxn) == (want.tokens, want.types, len(want), want.maxn), what
    for n in range(1, maxlength + 1):
        assert (st.found[n], st.pruned[n], st.kept[n]) == want.stats[n], (what, n)
    return st


def test_the_corpus_is_what_the_cases_need():
    """more than 256 survivors below class 4096 (hot and sorted unigram lists), cold ones from 9000 up, and lists of every order on both sides of token 65 536"""
    import oracle
    payload = corpus(101, 70000)
    assert sentence_count(payload) == 101 and payload[-1] != 0 and b"\x00\x00" in corpus(65534, 40000)  # (an unterminated last sentence; empty ones)
    want = _oracle(payload, tuple(sorted(KINDS["indexed"].items())))
    uni = [sum((b & 127) << (7 * i) for i, b in enumerate(k)) for k in want.counts if oracle.key_ntokens(k) == 1]
    assert sum(c < 4096 for c in uni) > 256 and sum(c >= 9000 for c in uni) >= 40
    for n in (1, 2, 3):  # the long sentence is number 51: a (51, t) that a list holds twice is one occurrence below token 65 536 and one above
        assert any(oracle.key_ntokens(k) == n and len({x for x in r if x[0] == 51}) < sum(x[0] == 51 for x in r) for k, r in want.refs.items()), n


# ---- a. natural shapes at every edge of the rule --------------------------------------------------------------------------------------------------------------
SHAPES = [  # sentences, longest, expected form (sb + tb)
    (65534, 40000, SPLIT),       # 16 + 16
    (65535, 40000, WHOLE),       # 17 + 16
    (131070, 40000, WHOLE),      # 17 + 16, the last sentence count with 17 bits
    (131071, 40000, UNPACKED),   # 18 + 16
    (131071, 32767, WHOLE),      # 18 + 15
    (131071, 32768, UNPACKED),   # 18 + 16
]
A_CASES = [(ns, lg, form, kind) for ns, lg, form in SHAPES for kind in ["indexed", "skipgrams", "order1_class"] + (["thr3"] if form != SPLIT else [])]


@pytest.mark.parametrize("nsent,longest,form,kind", A_CASES, ids=[f"{ns}x{lg}-{form}-{kind}" for ns, lg, form, kind in A_CASES])
def test_every_form_is_reached_by_corpus_shape_alone(ctx, nsent, longest, form, kind):
    """both sides of each edge of the sb / tb rule, by the corpus' own sentence count and longest sentence: the form the run reports, and the oracle's model"""
    payload = corpus(nsent, longest)
    assert sentence_count(payload) == nsent
    st = compare(ctx, payload, KINDS[kind], f"{nsent} sentences, longest {longest}, {kind}")
    assert form_of(st) == form


# ---- b. the token wrap ------------------------------------------------------------------------------------------------------------------------------------------
WRAP = [  # sentences, long sentences, form
    (101, (65535,), SPLIT),        # no wrap
    (101, (65536,), WHOLE),        # tb = 16 by the longest >= 65536 branch; no wrapped offset yet, but the whole word is the key from here on
    (101, (65537,), WHOLE),        # exactly one wrapped reference per order
    (101, (70000,), WHOLE),
    (102, (70000, 140000), WHOLE),  # wraps twice: (s, t) pairs that occur two and three times in a list
    (65535, (70000,), WHOLE),      # 17 + 16: whole by shape as well
]
B_CASES = [(ns, longs, form, kind) for ns, longs, form in WRAP for kind in ("indexed", "skipgrams", "order1_class")]


@pytest.mark.parametrize("nsent,longs,form,kind", B_CASES, ids=[f"{ns}x{'+'.join(map(str, lg))}-{kind}" for ns, lg, form, kind in B_CASES])
def test_lists_of_sentences_beyond_65536_tokens_are_in_the_references_order(ctx, nsent, longs, form, kind):
    """(sentence, token mod 65536) order, not corpus order: n-grams, skipgrams and the class-form order 1 alike"""
    payload = corpus(nsent, *longs)
    assert sentence_count(payload) == nsent
    st = compare(ctx, payload, KINDS[kind], f"{nsent} sentences, long ones {longs}, {kind}")
    assert form_of(st) == form
    if max(longs) >= 70000:  # (lists with the same (sentence, token) more than once: occurrences on both sides of a wrap)
        want = _oracle(payload, tuple(sorted(KINDS[kind].items())))
        assert any(len(set(r)) != len(r) for r in want.refs.values())


@pytest.mark.parametrize("kind", ["indexed", "skipgrams", "order1_class"])
def test_a_wrapping_sentence_among_more_than_131070_sentences_is_refused(ctx, kind):
    """sb = 18 and tb = 16 leave no room for whole pairs, and pairs that carry positions cannot be sorted into the reference's order: COLIBRI_ERR_UNSUPPORTED with the
    cause, no model in another order — and the context trains the next corpus as if nothing had happened"""
    from colibri_amd import capi
    payload = corpus(131071, 70000)
    assert sentence_count(payload) == 131071
    kw = dict(KINDS[kind])
    ctx.upload(payload, first_sentence=kw.pop("firstsentence", 1))
    with pytest.raises(capi.ColibriError) as e:
        ctx.train(mintokens=2, **kw)
    assert e.value.code == capi.ERR_UNSUPPORTED and "65536 tokens" in str(e.value) and "131070 sentences" in str(e.value)
    kw.pop("indexed")  # the same corpus, unindexed (the exhaustive kind where skipgrams were asked for), is no such case
    if kw.pop("doskipgrams", 0):
        kw["doskipgrams_exhaustive"] = 1
    ctx.train(mintokens=2, **kw)
    st = compare(ctx, corpus(101, 70000), KINDS[kind], "after a refusal")
    assert form_of(st) == WHOLE


# ---- c. forced forms on content-rich corpora -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rich_hot():
    from test_gpu_parity import _hot_refs_corpora
    return _hot_refs_corpora()


@functools.lru_cache(maxsize=None)
def _rich_small():
    return small_corpora()


def rich_corpus(name, hamlet):
    return hamlet if name == "hamlet" else _rich_hot()[name] if name == "zipf_6000" else _rich_small()[name]


SWITCHES = [(None, SPLIT), ("COLIBRI_WHOLE_PAIRS", WHOLE), ("COLIBRI_UNPACKED_PAIRS", UNPACKED), ("COLIBRI_NO_DIRECT_PAIRS", SPLIT), ("COLIBRI_NO_DIRECT_PAIRS2", SPLIT),
            ("COLIBRI_EXACT_RANKS", SPLIT), ("COLIBRI_NO_CHAIN_IDS", SPLIT), ("COLIBRI_ALL_IDS", SPLIT)]
RICH_KINDS = {"indexed_l5": dict(indexed=1, maxlength=5), "skipgrams_l4": dict(indexed=1, doskipgrams=1, maxlength=4)}
C_CASES = [(name, kind, switch, form) for name in ("zipf200k_phrases", "hamlet", "zipf_6000") for kind in RICH_KINDS for switch, form in SWITCHES]  # (switches innermost: one oracle run per corpus and kind)


@pytest.mark.parametrize("name,kind,switch,form", C_CASES, ids=[f"{n}-{k}-{(s or 'default').replace('COLIBRI_', '').lower()}" for n, k, s, f in C_CASES])
def test_forced_forms_and_emission_routes_give_the_oracles_lists(ctx, hamlet_payload, monkeypatch, name, kind, switch, form):
    """the switches that send a corpus through another pair form or another way of emitting its pairs (all read at every train()): each run against the oracle"""
    for s, _ in SWITCHES[1:]:
        monkeypatch.delenv(s, raising=False)
    if switch:
        monkeypatch.setenv(switch, "1")
    st = compare(ctx, bytes(rich_corpus(name, hamlet_payload)), RICH_KINDS[kind], f"{name}, {kind}, {switch or 'default'}")
    assert form_of(st) == form


# ---- d. sharded ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nsent,longest", [(101, 70000), (131071, 40000), (131071, 70000)], ids=["split_shape_wrap", "unpacked_shape", "unpacked_shape_wrap"])
def test_two_ranks_lists_joined_in_rank_order_are_the_oracles(nsent, longest):
    """capi.ShardedTrainer over two ranks of one device: every rank chooses the form its own share of the sentences asks for (a half of 131 071 sentences leaves room
    for whole pairs, so the wrapping sentence one device refuses is served here); the ranks' runs of a pattern joined in rank order are the oracle's list"""
    from colibri_amd import capi
    from colibri_amd.dist import merge_exports
    payload = corpus(nsent, longest)
    want = _oracle(payload, tuple(sorted(KINDS["indexed"].items())))
    with capi.ShardedTrainer(2, devices=[0, 0]) as tr:
        tr.upload_split(payload)
        tr.train(mintokens=2, maxlength=3, indexed=1)
        counts, refs = merge_exports([tr.export_local(r) for r in range(2)])
    compare_lists(counts, refs, want, f"two ranks, {nsent} sentences, longest {longest}")


# ---- e. the CLI ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_cli_model_of_a_wrapping_sentence_is_the_one_the_reference_loads(tmp_path):
    """colibri-patternmodeller builds the indexed model of the 70 000-token corpus; the file holds the oracle's model, and the real reference loads the same"""
    import oracle
    from colibri_amd import synth
    from test_host_face import CLI, parse_model
    payload = corpus(101, 70000)
    data, model = str(tmp_path / "c.colibri.dat"), str(tmp_path / "m.colibri.patternmodel")
    with open(data, "wb") as f:
        f.write(synth.HEADER + payload)
    out = subprocess.run([CLI, "-f", data, "-t", "2", "-l", "3", "-o", model], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    want = _oracle(payload, tuple(sorted(KINDS["indexed"].items())))
    mtype, tokens, types, counts, refs = parse_model(model)
    assert (mtype, tokens, types) == (20, want.tokens, want.types)
    compare_lists(counts, refs, want, "the CLI's model file")
    if oracle.have_ref():
        dump = str(tmp_path / "d.txt")
        subprocess.check_call([oracle.REF_DRIVER, "load", model, "i", dump])
        got = oracle.parse_dump(open(dump).read(), indexed=True)
        assert (got.tokens, got.types) == (want.tokens, want.types)
        compare_lists(got.counts, got.refs, want, "the reference's dump of the CLI's model file")
