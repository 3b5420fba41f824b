"""Flexgram abstraction on the device (csrc/flexgrams.hpp behind colibri_flexgrams / colibri_flexgrams_resident / colibri_flexgrams_fetch in
csrc/flex_api.inc) against the vectorised restatement tests/flex_models.py::restate, which tests/test_flexgrams.py pins to the oracle — at
the sizes where the scans, the radix sort and the grid-stride loops of the pipeline change path, with the group order, the order of the
merged lists and their duplicates compared exactly: all six fetched arrays, np.array_equal, no dicts and no tolerance.

ONE context serves the whole file, large and tiny models in turn: that a context may be used again is part of what is tested."""
import numpy as np
import pytest

import flex_models as fm

pytestmark = pytest.mark.gpu

SCAN_BLOCK = 1024          # csrc/kernels.hpp scan_reduce_kernel / scan_apply_kernel: `blockIdx.x * kBlock * 4` inputs per block
SCAN_CHUNK = 256 * 1024    # csrc/kernels.hpp scan_sums_kernel: `for (base = 0; base < nblocks; base += kBlock)` — 256 block sums per round of the carry
SORT_TILE = 4096           # csrc/kernels.hpp `constexpr int kSortTile = 4096`
SORT_CHUNK = 4096 * 1024   # csrc/colibri_hip.hip radix_sort_pairs: `nh = 256u * nblocks` histogram words through the same scan: 1024 tiles fill its first chunk
GRID = 4096 * 256          # csrc/colibri_hip.hip stream_grid: at most `256ull * 16` blocks of kBlock = 256 threads

NAMES = ("key_off", "key_bytes", "counts", "ref_off", "ref_sentence", "ref_token")
EDGE_TOKENS = [0, 255, 256, 65535]


@pytest.fixture(scope="module")
def ctx():
    from colibri_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def same(got, want, tag=None):
    """all six arrays, exactly (type, length, every element)"""
    fo, fk, fc, (fro, frs, frt) = got
    for name, g, w in zip(NAMES, (fo, fk, fc, fro, frs, frt), want):
        assert g.dtype == w.dtype and g.shape == w.shape, (tag, name, g.dtype, w.dtype, g.shape, w.shape)
        if not np.array_equal(g, w):
            at = int(np.flatnonzero(g != w)[0])
            raise AssertionError((tag, name, "first difference at", at, "device", g[at:at + 8].tolist(), "restatement", w[at:at + 8].tolist()))
    return fo, fk, fc, fro, frs, frt


def check(ctx, model, tag=None):
    return same(ctx.flexgrams(*model), fm.restate(*model), tag)


def split_unevenly(rng, total, parts):
    """`parts` counts that sum to `total`; uneven, zeros allowed"""
    cuts = np.sort(rng.integers(0, total + 1, size=parts - 1))
    return np.diff(np.concatenate(([0], cuts, [total])))


def spread_sentences(rng, n, top):
    """n sentence numbers in 0..top, every byte that `top` uses drawn at random, `top` itself, 0 and the values beside top's byte edges among them"""
    s = rng.integers(0, top, size=n, dtype=np.uint64, endpoint=True)
    plant = [v for v in (0, top, top - 1, top >> 8, top >> 16, 255, 256, 65535, 65536, (1 << 24) - 1, 1 << 24) if 0 <= v <= top]
    s[rng.choice(n, size=len(plant), replace=False)] = plant
    return s.astype(np.uint32)


# ---- a. scan edges over patterns ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("every", [1, 3], ids=["all_skipgrams", "every_third"])
@pytest.mark.parametrize("npat", [1, 2, SCAN_BLOCK - 1, SCAN_BLOCK, SCAN_BLOCK + 1, 2 * SCAN_BLOCK - 1, 2 * SCAN_BLOCK, 2 * SCAN_BLOCK + 1,
                                  SCAN_CHUNK - 1, SCAN_CHUNK, SCAN_CHUNK + 1, 2 * SCAN_CHUNK + 1])
def test_scan_edges_over_patterns(ctx, npat, every):
    """singletons with one reference each: flen, isrep and contrib are scanned over npat patterns, fx.cnt and glen over G groups. every = 1:
    G == npat, both cross together; every = 3: G = ceil(npat / 3), the group scans cross their block and chunk edges at other sizes than the
    pattern scans (the other patterns are n-grams, with a reference each too)"""
    rng = np.random.default_rng(100 + npat + every)
    keys, isskip = fm.singleton_block(npat, every)
    s, t = fm.draw_refs(rng, npat, (1, 200))
    model = fm.assemble(keys, np.ones(npat, dtype=np.int64), s, t, rng.permutation(npat))
    fo, fk, fc, fro, frs, frt = check(ctx, model, (npat, every))
    assert fc.size == int(isskip.sum()) == -(-npat // every) and fro[-1] == fc.size


# ---- b. sort tile and chunk edges over references ----------------------------------------------------------------------------------------
def one_group_of_8(rng, nf, sentences):
    pats = fm.fanin(6, 7, 8) + fm.distractors(6, 7)
    counts = np.concatenate((split_unevenly(rng, nf, 8), [2, 1, 3]))
    rng.shuffle(counts[:8])
    return fm.build(rng, pats, counts, sentences)[0]


@pytest.mark.parametrize("nf", [1, 63, 64, 65, 255, 256, 257, SORT_TILE - 1, SORT_TILE, SORT_TILE + 1, 2 * SORT_TILE - 1, 2 * SORT_TILE + 1, 4 * SORT_TILE + 1])
def test_sort_tile_edges_over_references(ctx, nf):
    """one fan-in group of 8 members (and three patterns that are no skipgrams) with nf references in all: the lanes of a wave, the waves of a
    row, the rows of a tile, the tiles"""
    rng = np.random.default_rng(200 + nf)
    fo, fk, fc, fro, frs, frt = check(ctx, one_group_of_8(rng, nf, (1, 3000)), nf)
    assert fc.tolist() == [nf]


@pytest.mark.parametrize("nf", [SORT_CHUNK, SORT_CHUNK + 1])
def test_sort_histogram_scan_crosses_its_chunk(ctx, nf):
    """nf = SORT_CHUNK + 1 references make 1025 tiles = 262 400 histogram words = 257 block sums: the carry of scan_sums_kernel acts inside
    radix_sort_pairs. 11 patterns; the cost is the references (the restatement's lexsort of 4.2 M triples is the bulk of this test)"""
    rng = np.random.default_rng(300 + nf - SORT_CHUNK)
    fo, fk, fc, fro, frs, frt = check(ctx, one_group_of_8(rng, nf, (1, 70000)), nf)
    assert fc.tolist() == [nf]


# ---- c. pass counts ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("top", [0, 1, 255, 256, 65535, 65536, (1 << 24) - 1, 1 << 24, (1 << 32) - 1])
def test_sentence_pass_counts(ctx, top):
    """the sentence sort runs bits_for(largest sentence + 1) bits: 1 .. 4 passes. 300 groups, 20 000 references whose sentences use every byte
    that `top` uses — a dropped pass, or one that reads digits above `bits`, mis-orders them"""
    rng = np.random.default_rng(400 + top % 1000)
    pats = [p for i in range(300) for p in fm.singleton(200 + i, 7)]
    counts = split_unevenly(rng, 20000, 300)
    s = spread_sentences(rng, 20000, top)
    t = rng.choice(np.array(EDGE_TOKENS + [1, 257, 511, 512, 65280], dtype=np.uint16), size=20000)
    model, _ = fm.build(rng, pats, counts, refs=(s, t), plant=False)  # (nine tokens: equal pairs come by themselves where the sentences are few)
    fo, fk, fc, fro, frs, frt = check(ctx, model, top)
    assert frs.max() == top and set(EDGE_TOKENS) <= set(frt.tolist())


@pytest.mark.parametrize("G", [1, 2, 255, 256, 257, 65535, 65536, 65537])
def test_group_pass_counts(ctx, G):
    """the group sort runs bits_for(G) bits: 1 .. 3 passes, with edges at 256 / 257 and 65 536 / 65 537 groups; three references per group,
    sentences below 256"""
    rng = np.random.default_rng(500 + G)
    keys, _ = fm.singleton_block(G)
    s = rng.integers(0, 256, size=3 * G, dtype=np.uint32)
    t = rng.choice(np.array(EDGE_TOKENS, dtype=np.uint16), size=3 * G)
    t[:min(4, 3 * G)] = EDGE_TOKENS[:min(4, 3 * G)]
    model = fm.assemble(keys, np.full(G, 3), s, t, rng.permutation(G))
    fo, fk, fc, fro, frs, frt = check(ctx, model, G)
    assert fc.size == G and fro[-1] == 3 * G
    assert set(EDGE_TOKENS[:3 * G]) <= set(frt.tolist())


# ---- d. stability ------------------------------------------------------------------------------------------------------------------------
def test_stability_across_lanes_waves_rows_and_tiles(ctx):
    """four groups of 5000 .. 70 000 references among 300 small ones. Few distinct sentences, and tokens that differ only in their high or only
    in their low byte: the merged lists come out ascending only if every pass keeps the order of the pass before it, in every lane, wave,
    row and tile. Thousands of references are the same (sentence, token) pair in different members."""
    rng = np.random.default_rng(600)
    pats, counts = [], []
    for j, size in enumerate([5000, 17000, 40000, 70000]):
        pats += fm.fanin(300 + j, 9, 7)
        counts += split_unevenly(rng, size, 7).tolist()
    for j in range(300):
        pats += fm.singleton(400 + j, 10) if j % 3 else fm.fanin(400 + j, 10, 2)
    counts += rng.integers(0, 9, size=len(pats) - len(counts)).tolist()
    n = int(np.sum(counts))
    s = rng.integers(1, 13, size=n, dtype=np.uint32) * np.uint32(257)  # 12 sentences whose two low bytes are equal
    tokens = np.array([h << 8 for h in range(0, 256, 5)] + list(range(0, 256, 7)) + [h << 8 | 255 for h in range(3)] + EDGE_TOKENS, dtype=np.uint16)
    t = rng.choice(tokens, size=n)
    model, _ = fm.build(rng, pats, counts, refs=(s, t))
    fo, fk, fc, fro, frs, frt = check(ctx, model)
    big =np.sort(fc)[-4:].tolist()
    assert big == [5000, 17000, 40000, 70000] and fc.size == 304
    pairs = frs.astype(np.uint64) << np.uint64(16) | frt
    assert int((np.diff(pairs) == 0).sum()) > 100000, "equal pairs, from different members, are kept"


def test_every_reference_the_same_pair(ctx):
    rng = np.random.default_rng(601)
    pats = fm.fanin(6, 7, 5) + fm.singleton(8, 9) + fm.fanin(10, 11, 3) + fm.distractors(6, 7)
    counts = [3000, 1, 0, 9000, 4097, 1, 300, 0, 5000, 7, 7, 7]
    n = sum(counts)
    model, _ = fm.build(rng, pats, counts, refs=(np.full(n, 258), np.full(n, 513)))
    fo, fk, fc, fro, frs, frt = check(ctx, model)
    assert sorted(fc.tolist()) == [1, 5300, 16098] and set(frs.tolist()) == {258} and set(frt.tolist()) == {513}


# ---- e. ownership of references ----------------------------------------------------------------------------------------------------------
def ownership_model(rng, skip_refs=True, ngram_refs=True):
    """patterns without references at number 0 and at the end, in runs of 1, 2, 1024 and 1025, directly before and after a pattern with one
    reference and around one with 5000; skipgrams and n-grams are empty alike. Not shuffled: the places are the point."""
    words = iter(range(200, 20000))

    def some(n, count, start=0):
        """n patterns of `count` references each: a singleton skipgram, an n-gram, a member of a group of two, an n-gram, and so on"""
        out, shared = [], None
        for j in range(start, start + n):
            if j % 2:
                out.append(((fm.encode([next(words), 6]), None), count if ngram_refs else 0))
                continue
            if j % 4 == 0:
                p = fm.singleton(next(words), 6)[0]
            else:
                shared = next(words) if j % 8 == 2 or shared is None else shared
                p = fm.fanin(shared, 6, 2)[(j % 8) // 4]
            out.append((p, count if skip_refs else 0))
        return out

    rows = some(1, 0) + some(3, 1) + some(2, 0) + some(1, 1) + some(2, 0) + some(1, 1, start=1) + some(2, 0) + some(3, 5000) + some(1, 0) + some(1, 5000) + some(3, 0) + some(2, 2)
    rows += some(1024, 0) + some(2, 1) + some(1025, 0) + some(3, 3) + some(1, 0, start=1) + some(1, 1) + some(1, 0)
    pats, counts = [p for p, _ in rows], [c for _, c in rows]
    assert counts[0] == 0 and counts[-1] == 0
    return fm.build(rng, pats, counts, (1, 500), shuffle=False)[0]


def test_ownership_of_references_around_empty_patterns(ctx):
    fo, fk, fc, fro, frs, frt = check(ctx, ownership_model(np.random.default_rng(700)))
    assert (fc == 0).sum() > 700 and (fc >= 5000).sum() >= 3


def test_only_ngrams_have_references(ctx):
    """nf == 0 with G > 0: the keys come back, no sort runs"""
    fo, fk, fc, fro, frs, frt = check(ctx, ownership_model(np.random.default_rng(701), skip_refs=False))
    assert fc.size > 700 and not fc.any() and frs.size == 0 and frt.size == 0 and fk.size > 0


def test_every_pattern_without_references(ctx):
    fo, fk, fc, fro, frs, frt = check(ctx, ownership_model(np.random.default_rng(702), skip_refs=False, ngram_refs=False))
    assert fc.size > 700 and not fc.any() and frs.size == 0


@pytest.mark.parametrize("nr_in", [GRID - 1, GRID, GRID + 1, 2 * GRID + 5])
def test_reference_grid_stride(ctx, nr_in):
    """flex_ref_list_kernel walks nr_in references with 4096 blocks of 256 threads: beyond GRID references its loop runs again, for some
    threads only, and every lane must still reach the wave reduction of the largest sentence (which lies in the last reference of a
    skipgram here). 600 patterns, skipgrams and n-grams in turn, so that about half of the references are sorted."""
    rng = np.random.default_rng(800 + nr_in - GRID)
    pats = []
    for j in range(300):
        pats += [(fm.encode([200 + j, 6]), None)] + fm.singleton(200 + j, 6)
    counts = split_unevenly(rng, nr_in, 600)
    counts[-1] += counts[-2]  # pattern 599 is a skipgram: it holds the last references
    counts[-2] = 0
    s, t = fm.draw_refs(rng, nr_in, (1, 60000))
    s[-1] = 16_000_000  # three sentence passes, asked for by the last reference alone
    model, _ = fm.build(rng, pats, counts, refs=(s, t), shuffle=False, plant=False)
    fo, fk, fc, fro, frs, frt = check(ctx, model, nr_in)
    assert counts[-1] > 0 and 0.4 * nr_in < fro[-1] < 0.6 * nr_in and frs.max() == 16_000_000


# ---- f. categories and bytes -------------------------------------------------------------------------------------------------------------
def test_categories_and_bytes(ctx):
    """the multi-byte, long and distractor families together, 4000 patterns: the classes at the varint edges, classes with 03 / 04 / 83 / 84
    among their bytes, keys of 100 and more tokens, keys that begin or end with a gap or are gaps only, n-grams, patterns that hold a {**},
    and flexgrams that some group's key equals — whose references (sentence 4 000 000 000 and up) must not come back"""
    rng = np.random.default_rng(900)
    pats = dict(fm.long_keys(rng, 6))
    words = [int(w) for w in rng.permutation(fm.VOCAB)]
    for a in words:
        for b in words[:12]:
            for k, g in (fm.fanin(a, b, 3) if (a + b) % 3 else fm.singleton(a, b)) + fm.distractors(a, b):
                pats.setdefault(k, g)
    while len(pats) < 4000:
        for k, g in fm.multibyte(rng, 4000 - len(pats)):
            pats.setdefault(k, g)
    pats = list(pats.items())
    counts = rng.integers(0, 6, size=len(pats))
    off = np.concatenate(([0], np.cumsum(counts)))
    s, t = fm.draw_refs(rng, int(off[-1]), (1, 100000))
    groupkeys = {g for _, g in pats if g is not None}
    preexisting = [i for i, (k, g) in enumerate(pats) if k in groupkeys]
    assert len(preexisting) > 100 and len(pats) == 4000
    for i in preexisting:
        s[off[i]: off[i + 1]] = 4_000_000_000 + i
    model, groups = fm.build(rng, pats, counts, refs=(s, t))
    fo, fk, fc, fro, frs, frt = check(ctx, model)
    assert fc.size == len(groups) == len(groupkeys) and frs.size and frs.max() < 4_000_000_000
    kb = fk.tobytes()
    keys = [kb[a:b] for a, b in zip(fo[:-1].tolist(), fo[1:].tolist())]
    assert keys == [g for g, _ in groups]
    assert all(b"\x03" not in fm.tokens_of(k) and b"\x04" in fm.tokens_of(k) for k in keys), "no gap is left in a flexgram"
    assert any(len(fm.tokens_of(k)) >= 100 for k in keys) and bytes([fm.FLEX]) in keys


# ---- g. group order and representatives --------------------------------------------------------------------------------------------------
def test_group_order_and_representatives(ctx):
    """300 000 patterns; 500 fan-in groups of 8 whose lowest member is the last thread of a late block (pattern 255 mod 256) while the seven
    others are first threads of the blocks after it: whichever of them reaches the table first, the representative is the lowest, and the
    groups are numbered by it. Three calls on one context give the same arrays."""
    rng = np.random.default_rng(1000)
    npat = 300_000
    keys, isskip = fm.singleton_block(npat, every=2)  # every second filler is a group of its own, between the fan-in groups' members
    keys = [bytes(r) for r in keys]
    for j in range(500):
        block = 100 + 2 * j
        members = fm.fanin(20000 + j, 6, 8)
        rng.shuffle(members)
        # (groups whose blocks overlap are fewer than four apart: j % 4 keeps their places distinct)
        for k, place in zip(members, [256 * block + 255] + [256 * (block + 1 + int(d)) + 8 * (j % 4) + int(x) for d, x in zip(rng.permutation(7), rng.integers(0, 8, size=7))]):
            keys[place], isskip[place] = k[0], False
    assert len(set(keys)) == npat
    counts = rng.integers(0, 3, size=npat)
    s, t = fm.draw_refs(rng, int(counts.sum()), (1, 1000))
    model = fm.assemble(keys, counts, s, t)
    want = fm.restate(*model)
    first = same(ctx.flexgrams(*model), want)
    assert first[2].size == int(isskip.sum()) + 500
    for again in range(2):
        same(ctx.flexgrams(*model), first, again)


# ---- h. forced collisions at size --------------------------------------------------------------------------------------------------------
def test_forced_collisions_at_size(ctx, monkeypatch):
    """20 000 groups under 12 bits of hash: the first two attempts collide, the third is unmasked; the answer is the one without the switch"""
    rng = np.random.default_rng(1100)
    keys, _ = fm.singleton_block(20000)
    keys = [bytes(r) for r in keys] + [k for j in range(300) for k, _ in fm.fanin(20000 + j, 6, 4)]
    counts = rng.integers(0, 4, size=len(keys))
    s, t = fm.draw_refs(rng, int(counts.sum()), (1, 1000))
    model = fm.assemble(keys, counts, s, t, rng.permutation(len(keys)))
    want = fm.restate(*model)
    assert want[2].size == 20300
    same(ctx.flexgrams(*model), want, "no switch")
    monkeypatch.setenv("COLIBRI_FLEX_HASH_BITS", "12:2")
    same(ctx.flexgrams(*model), want, "12:2")
    monkeypatch.delenv("COLIBRI_FLEX_HASH_BITS")
    same(ctx.flexgrams(*model), want, "switch off again")


# ---- i. resident form --------------------------------------------------------------------------------------------------------------------
def test_resident_form_and_a_tiny_model_after_it(ctx):
    from conftest import small_corpora
    ctx.upload(small_corpora()["zipf200k_phrases"])
    ctx.train(mintokens=2, maxlength=7, indexed=1, doskipgrams=1, minskiptypes=1)
    key_off, key_bytes, _, (ref_off, rs, rt) = ctx.export_arrays()
    want = fm.restate(key_off, key_bytes, ref_off, rs, rt)
    assert want[2].size > 1000
    same(ctx.flexgrams_resident(), want, "resident")
    same(ctx.flexgrams(key_off, key_bytes, ref_off, rs, rt), want, "uploaded")
    # nothing of the large answer is left in the context when a model of three patterns follows
    tiny, _ = fm.build(np.random.default_rng(1200), fm.fanin(6, 7, 2) + [(fm.encode([6, 7]), None)], [2, 1, 4], (1, 9))
    fo, fk, fc, fro, frs, frt = check(ctx, tiny, "tiny")
    assert fk.tobytes() == bytes([6, 4, 7]) and fc.tolist() == [3]
