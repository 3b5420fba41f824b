"""GPU: the order-2 and chained kernels at their bin, list and tile edges (csrc/bigram2.hpp, csrc/chain.hpp; the driver around bigram2_plan, bigram2_order
and chain_order in csrc/colibri_hip.hip). The rest of the suite compares this engine with the oracle on DRAWN corpora, which land where the statistics put
them; the corpora here are BUILT (tests/bin_models.py, pinned by tests/test_bi2_mix.py) to stand on either side of the engine's structural constants:
the table of a final bin at 256 / 512 / 1024 slots, the register window of 768 records, 900 distinct keys, survivor rank 256, big bins (1536), the workgroup
kernel's bins (16 384; 4096 for orders >= 3), 16-bit counters at 32 768 and 65 536, full table buckets and the wrap at the table's end, a wave's position list,
the dense head's edge at class 64, lane 63, the 1024-thread row, the 4096-window tile, position buckets, the corpus' end, and the lists' lengths modulo 4.

Every case trains through the C ABI and is compared with the oracle's model of the same payload: patterns and counts, totals, found / pruned / kept per order,
and every reference of an indexed model. Equality throughout. Every case also asserts its premise — the order-2 records and head windows its builder intended
(Context.order2_records, after plain runs: an indexed run does not keep that figure; both assert the admitted windows), the engines that ran
(colibri_stats.path) and that the run was not repeated — or, where the case is built to make order 2 give up (one distinct key more than a table holds, one
window more than a wave's list, a quarter of a hot key's records more than a record slot: Bi2State.overflow 2, 3 and 1, all DevState.radix_overflow 4 and so
COLIBRI_FALLBACK_ORDER2), that it was, with the model still the
oracle's."""
import functools

import pytest

import bin_models as bm

pytestmark = pytest.mark.gpu

PLAIN_INDEXED = pytest.mark.parametrize("indexed", [False, True], ids=["plain", "indexed"])


@pytest.fixture(scope="module")
def ctx():
    from colibri_amd import capi
    with capi.Context(0) as c:
        yield c


_built = functools.lru_cache(maxsize=None)  # a corpus is built once per module, whatever runs on it


@_built
def _hot(n, copies, wcap_edge=False):
    return bm.hot_ngram(n, copies, wcap_edge=wcap_edge)


@_built
def _distinct(D, second=0):
    return bm.distinct_in_bin(D, second)


@_built
def _survivors(S, D, mintokens=2, low=None):
    return bm.survivors_in_bin(S, D, mintokens, low)


@_built
def _walk(n, lgb, last):
    return bm.bucket_walk(n, lgb, last)


@_built
def _aligned(s):
    return bm.aligned_text(s)


@_built
def _end(npos, closing):
    return bm.corpus_end(npos, closing)


@_built
def _lists(k):
    return bm.list_lengths(k)


@_built
def _head_edge():
    return bm.head_edge()


@functools.lru_cache(maxsize=None)
def _oracle(build, args, maxlength, indexed):
    import oracle
    corpus = build(*args).corpus
    return oracle.train(corpus.payload, corpus.mintokens, maxlength, indexed=indexed)


def run(ctx, build, args, maxlength, indexed, profile=0):
    """train the case's corpus, compare the model with the oracle's, assert the case's premise"""
    from colibri_amd import capi
    case = build(*args)
    corpus = case.corpus
    want = _oracle(build, args, maxlength, indexed)
    ctx.upload(corpus.payload)
    assert ctx.positions() == corpus.npos
    st = ctx.train(mintokens=corpus.mintokens, maxlength=maxlength, indexed=int(indexed), profile=profile)
    got, gotrefs = ctx.export_dict()
    # the model
    assert got == want.counts
    if indexed:
        assert gotrefs == want.refs
    assert (st.totaltokens, st.totaltypes, st.maxn, st.npatterns) == (want.tokens, want.types, want.maxn, len(want.counts))
    for n in range(1, maxlength + 1):
        assert (st.found[n], st.pruned[n], st.kept[n]) == want.stats[n], n
    assert sum(st.windows[1:min(maxlength, want.maxn + 1) + 1]) == want.windows
    # the premise: this run reached its edge
    if case.gives_up:
        assert st.fallback_reason == case.reason and st.retries >= 1, (st.fallback_reason, st.retries)
    else:
        assert (st.fallback_reason, st.retries) == (0, 0)
        assert st.path & capi.PATH_BI2, st.path
        assert maxlength < 3 or st.path & capi.PATH_CHAIN, st.path
        if not indexed:  # (colibri_order2_records answers after plain runs only: an indexed case rests on the admitted windows below and on the plain run of the same corpus,
            assert ctx.order2_records() == (case.records, case.head)  # which every family has — that run pins the edge the indexed one then stands on)
        if profile:  # order 2 on the second-generation count kernels, the orders >= 3 that ran on the chained ones, and no order a second time on the first generation
            assert ctx.kernel_time(capi.K_COUNT2)[1] >= 1 and ctx.kernel_time(capi.K_BINCOUNT)[1] == max(0, min(maxlength, want.maxn + 1) - 2), \
                (ctx.kernel_time(capi.K_COUNT2), ctx.kernel_time(capi.K_BINCOUNT))
    assert st.admitted[2] == case.records + case.head
    return st, case


# ---- a. one hot bigram in a bin of its own ---------------------------------------------------------------------------------------------------------------
# the table's growth (total + total / 2 against 256 and 512 slots), the register window, the big bins' list
HOT_LISTED = [170, 171, 172, 341, 342, 767, 768, 769, 1535, 1536, 1537]
# a plain run to length 2 asks bigram2_order for no position lists (want_list = n < maxlength), so nothing bounds the count but the record slots — the builder
# appends empty sentences until one slot holds a quarter of the hot bigram's records (Corpus' pad_region): the workgroup kernel's bins, the 16-bit counters' ends
HOT_UNLISTED = [4095, 4096, 4097, 16383, 16384, 16385, 32767, 32768, 32769, 65535, 65536, 65537]


@pytest.mark.parametrize("maxlength,indexed", [(3, False), (2, True)], ids=["plain-3", "indexed-2"])
@pytest.mark.parametrize("copies", HOT_LISTED)
def test_hot_bigram_with_lists(ctx, copies, maxlength, indexed):
    run(ctx, _hot, (2, copies), maxlength, indexed, profile=1)


@pytest.mark.parametrize("maxlength,indexed", [(3, False), (2, True)], ids=["plain-3", "indexed-2"])
@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_hot_bigram_at_the_waves_list_capacity(ctx, delta, maxlength, indexed):
    """the bin's wave lists every window of the surviving bigram: wcap(npos) entries fit, one more makes order 2 give up (Bi2State.overflow 3)"""
    copies = bm.hot_copies_for_wcap(delta)
    _, case = run(ctx, _hot, (2, copies, True), maxlength, indexed, profile=1)
    assert copies == bm.wcap(case.corpus.npos) + delta and case.gives_up == (delta > 0)


@functools.lru_cache(maxsize=1)  # (millions of positions each: not kept)
def _hot_padded(copies):
    return bm.hot_ngram(2, copies)


@pytest.mark.parametrize("copies", HOT_UNLISTED)
def test_hot_bigram_without_lists(ctx, copies):
    _, case = run(ctx, _hot_padded, (copies,), 2, False, profile=1)
    assert bm.region(case.corpus.npos) >= copies // 4


@functools.lru_cache(maxsize=1)
def _hot_unpadded(copies):
    return bm.hot_ngram(2, copies, pad_region=False)


def test_hot_bigram_that_overruns_its_record_slot():
    """without the padding a quarter of 65 537 records does not fit a (sub-region, A bin) slot of 4096: Bi2State.overflow 1, which order 2's finish kernel passes on as
    DevState.radix_overflow 4 like its other two, so the run repeats without the second-generation order 2 (COLIBRI_FALLBACK_ORDER2, train_retry.hpp) and the model is
    still the oracle's. On a context of its own: device arrays only grow,
    and the module's context has held corpora whose record arrays would take these records"""
    from colibri_amd import capi
    with capi.Context(0) as fresh:
        _, case = run(fresh, _hot_unpadded, (65537,), 2, False)
    assert case.gives_up and case.reason == capi.FALLBACK_ORDER2 and bm.region(case.corpus.npos) == 4096


# ---- b. distinct keys in one bin ---------------------------------------------------------------------------------------------------------------------------
@PLAIN_INDEXED
@pytest.mark.parametrize("D", [171, 172, 341, 342, 767, 768, 769, 899, 900, 901])
def test_distinct_keys_in_one_bin(ctx, D, indexed):
    """D bigrams once each: the table sizes, the register window, and kBi2MaxLoad — 900 distinct keys are counted, 901 make order 2 give up (overflow 2)"""
    _, case = run(ctx, _distinct, (D,), 3, indexed)
    assert case.bins[bm.BIN1] == (D, D, 0) and case.gives_up == (D > 900)


@PLAIN_INDEXED
def test_two_full_bins_next_to_each_other(ctx, indexed):
    """600 distinct keys in a bin and 600 more in the bin eight further on in the count kernel's walk, the next one of the same queue: two full bins side by side
    (which wave draws which is the scheduler's: nothing makes one wave take both)"""
    _, case = run(ctx, _distinct, (600, 600), 3, indexed)
    assert bm.walk_index(bm.BIN2) == bm.walk_index(bm.BIN1) + 8 and case.bins[bm.BIN2] == (600, 600, 0)


# ---- c. survivors in one bin -------------------------------------------------------------------------------------------------------------------------------
# (S, D, mintokens, copies of the others): survivor ranks on either side of 256 (representatives in LDS below, device atomics from there), ranked from the registers
# (at most 768 records) or by the slot sweep (more). D = 520 where the issue says 500: S + 500 records pass 768 only from S = 269. With mintokens 3 a bin of 257
# survivors has at least 771 records, so the direct ranking is held at S = D = 256 (768 records exactly) and the sweep at 3 copies against 2.
SURVIVORS = [(255, 300, 2, None, False), (256, 300, 2, None, False), (257, 300, 2, None, False),
             (255, 520, 2, None, True), (256, 520, 2, None, True), (257, 520, 2, None, True), (384, 520, 2, None, True),
             (256, 256, 3, None, False), (256, 300, 3, 2, True), (257, 300, 3, 2, True)]


@PLAIN_INDEXED
@pytest.mark.parametrize("S,D,mintokens,low,sweep", SURVIVORS, ids=[f"S{s}-D{d}-min{m}" for s, d, m, _, _ in SURVIVORS])
def test_survivors_in_one_bin(ctx, S, D, mintokens, low, sweep, indexed):
    _, case = run(ctx, _survivors, (S, D, mintokens, low), 3, indexed)
    records, distinct, kept = case.bins[bm.BIN1]
    assert (distinct, kept) == (D, S) and (records > bm.REG_WINDOW) == sweep, "the ranking this case is about"


# ---- d. table buckets --------------------------------------------------------------------------------------------------------------------------------------
@PLAIN_INDEXED
@pytest.mark.parametrize("last", [False, True], ids=["middle", "last-bucket"])
@pytest.mark.parametrize("lgb", [6, 7, 8], ids=["256-slots", "512-slots", "1024-slots"])
@pytest.mark.parametrize("n", [4, 5, 8, 9, 17])
def test_keys_that_start_in_one_bucket(ctx, n, lgb, last, indexed):
    """a bucket holds four keys: the fifth walks into the next bucket, the ninth into the one after, and from the table's last bucket the walk wraps to bucket 0"""
    _, case = run(ctx, _walk, (n, lgb, last), 3, indexed)
    assert bm.table_lgb(case.bins[bm.BIN1][0]) == lgb and (case.bucket == (1 << lgb) - 1) == last and len(case.chain) == n


# ---- e. orders >= 3, one hot n-gram ------------------------------------------------------------------------------------------------------------------------
@PLAIN_INDEXED
@pytest.mark.parametrize("maxlength", [3, 4])
@pytest.mark.parametrize("n", [3, 4], ids=["abc", "abcd"])
@pytest.mark.parametrize("copies", [767, 768, 769, 1535, 1536, 1537, 4095, 4096, 4097])
def test_hot_ngram_of_the_chained_orders(ctx, copies, n, maxlength, indexed):
    """the bins of the hot trigram (and 4-gram) at the register window, the big bins' list and kChHugeBin, beyond which a workgroup counts the bin"""
    _, case = run(ctx, _hot, (n, copies), maxlength, indexed, profile=1)
    assert copies <= bm.wcap(case.corpus.npos)


# ---- f. the head's edge ------------------------------------------------------------------------------------------------------------------------------------
@PLAIN_INDEXED
def test_classes_around_the_heads_edge(ctx, indexed):
    _, case = run(ctx, _head_edge, (), 3, indexed)
    assert case.head == 8  # (62 | 63) x (62 | 63): two surviving pairs with three windows each, two pairs with one


# ---- g. lane, row, tile and bucket alignment ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", range(65))
def test_text_at_every_lane_offset(ctx, s):
    """one text behind s + 1 positions that admit no window: every window once at each lane offset, the boundaries 63 | 64, 1023 | 1024 and 4095 | 4096 (a tile's
    end, a position bucket's end) crossed by surviving windows of every order"""
    run(ctx, _aligned, (s,), 4, False)


@pytest.mark.parametrize("s", range(0, 65, 4))
def test_text_at_every_fourth_lane_offset_indexed(ctx, s):
    run(ctx, _aligned, (s,), 4, True)


# ---- h. corpus ends ----------------------------------------------------------------------------------------------------------------------------------------
@PLAIN_INDEXED
@pytest.mark.parametrize("closing", [True, False], ids=["closed", "open"])
@pytest.mark.parametrize("npos", [4095, 4096, 4097, 8191, 8192, 8193])
def test_corpus_ends_in_a_surviving_trigram(ctx, npos, closing, indexed):
    _, case = run(ctx, _end, (npos, closing), 3, indexed)
    assert case.corpus.npos == npos


# ---- i. list lengths ---------------------------------------------------------------------------------------------------------------------------------------
@PLAIN_INDEXED
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 6, 7, 8, 9, 17])
def test_position_lists_of_every_length_modulo_four(ctx, k, indexed):
    """chain_bitmap_kernel reads a list in 16-byte groups and an n & 3 tail: k surviving windows in position bucket 0, k + 3 in bucket 1"""
    _, case = run(ctx, _lists, (k,), 3, indexed)
    assert sorted(case.lists.values()) == sorted([k, k, 3])
