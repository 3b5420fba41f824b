"""The bin arithmetic of the radix engine (csrc/bi2_mix.hpp, csrc/bigram2.hpp, csrc/chain.hpp and their driver in csrc/colibri_hip.hip), restated
in numpy, and corpora built with it: tests/test_gpu_bin_edges.py puts inputs on either side of the engine's structural constants BY CONSTRUCTION —
a final bin with exactly D distinct bigrams and S survivors, n keys that start in one bucket of a bin's LDS table, a hot bigram with exactly as many
windows as a wave's position list holds — instead of waiting for a Zipf draw to land there. tests/test_bi2_mix.py pins the restatement to the C++
(mix, bucket) and the builders to the oracle (a corpus means what its test says it means). Nothing here needs a device.

An order with fewer than ~1.4 M records has 8 B bins per A bin (bshift 6): 2048 final bins, and the final bin of a bigram is a pure function of its
two class ids (final_bin). With one n-gram per sentence the only windows of an order are the ones the test put there."""
import collections

import numpy as np

from colibri_amd import synth

# ---- the engine's constants (csrc/bigram2.hpp, csrc/chain.hpp, csrc/colibri_hip.hip) ----------------------------------------------------------------
MIX_C = (0x9E3779, 0x85EBCB, 0xC2B2AF, 0x27D4EB)  # kBi2MixC
HEAD = 64            # kBi2Head: classes below it on both sides are counted in the dense head and never become records
WAVE, ROWS = 64, 12  # bins of up to WAVE * ROWS records are ranked from registers, larger ones by a sweep over the table's slots
REG_WINDOW = WAVE * ROWS
BIG_BIN, HUGE_BIN, CH_HUGE_BIN = 1536, 16384, 4096  # kBi2BigBin, kBi2HugeBin, kChHugeBin
MAX_LOAD, SLOTS, REPS = 900, 1024, 256              # kBi2MaxLoad, kBi2WSlots, SLOTS / 4
TILE = 4096                                         # kBi2Tile: windows per emit tile; also the smallest position bucket
BINS, BBINS, BIN_TARGET = 256, 512, 700             # kBins, kBi2BBins, kBi2BinTarget
WAVES, EMIT_GRID, SUBS, SHARDS = 5120, 512, 4, 8    # kBi2Waves, kBi2EmitGrid, kBi2Sub, kBi2Shards
SCAT_TILE = 2048                                    # kScatTile (the floor of the record arrays: plan_buffers)
TOP = 4095                                          # the highest class of the corpora built here: clsbits 12, K = 24


def _f(r, c, outbits):
    return (((r & np.uint64(0xFFFFFF)) * np.uint64(c)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - outbits)


def _halves(K):
    h = K >> 1
    hb = K - h
    return h, min(h, 24), min(hb, 24)


def _as_u64(x):
    a = np.asarray(x, dtype=np.uint64)
    return a, a.ndim == 0


def mix(x, K):
    """bi2_mix: four Feistel rounds over the low K / 2 bits and the rest; ints or arrays of values below 2^K"""
    x, scalar = _as_u64(x)
    h, fl, fh = _halves(K)
    lo, hi = x & np.uint64((1 << h) - 1), x >> np.uint64(h)
    hi = hi ^ _f(lo, MIX_C[0], fh)
    lo = lo ^ _f(hi, MIX_C[1], fl)
    hi = hi ^ _f(lo, MIX_C[2], fh)
    lo = lo ^ _f(hi, MIX_C[3], fl)
    y = (hi << np.uint64(h)) | lo
    return int(y) if scalar else y


def unmix(y, K):
    """the rounds of mix() in reverse order"""
    y, scalar = _as_u64(y)
    h, fl, fh = _halves(K)
    lo, hi = y & np.uint64((1 << h) - 1), y >> np.uint64(h)
    lo = lo ^ _f(hi, MIX_C[3], fl)
    hi = hi ^ _f(lo, MIX_C[2], fh)
    lo = lo ^ _f(hi, MIX_C[1], fl)
    hi = hi ^ _f(lo, MIX_C[0], fh)
    x = (hi << np.uint64(h)) | lo
    return int(x) if scalar else x


def clsbits(maxclass):
    """bigram2_plan: bits of a class id"""
    b = 1
    while (1 << b) <= maxclass:
        b += 1
    return b


def order2_kbits(cb, sbits=0, kmin=0):
    """bi2_emit_kernel's head: key bits of order 2"""
    return max(2 * cb, 17 + sbits, kmin)


def bshift(records, K):
    """bi2_set_bshift: the B bin is the nine mix bits below the A bin, shifted down by this"""
    nb = 8
    while nb < BBINS and nb * BINS * BIN_TARGET < records:
        nb <<= 1
    sh = 0
    while (BBINS >> sh) > nb:
        sh += 1
    if sh + K > 48:
        sh = 0 if K >= 48 else 48 - K
    return sh


def bin_of_mix(m, K, bsh):
    """(A, B) of a mixed key"""
    m, scalar = _as_u64(m)
    a = (m >> np.uint64(K - 8)) & np.uint64(255)
    b = ((m >> np.uint64(K - 17)) & np.uint64(511)) >> np.uint64(bsh)
    return (int(a), int(b)) if scalar else (a, b)


def final_bin(a, b, cb=12, records=0):
    """the final bin (A, B) of the bigram (a, b) in an order of `records` records"""
    K = order2_kbits(cb)
    return bin_of_mix(mix((np.asarray(a, dtype=np.uint64) << np.uint64(cb)) | np.asarray(b, dtype=np.uint64), K), K, bshift(records, K))


def walk_index(fbin):
    """bi2_count_kernel's regular walk: bin g = B << 8 | A belongs to queue g & 7 — which is also the shard of the position lists its windows join"""
    return (fbin[1] << 8) | fbin[0]


def inbin_key(a, b, cb=12):
    """what a final bin's LDS table holds for the bigram: the K - 8 mix bits below the A bin, cut to 31 bits"""
    K = order2_kbits(cb)
    m, scalar = _as_u64(mix((np.asarray(a, dtype=np.uint64) << np.uint64(cb)) | np.asarray(b, dtype=np.uint64), K))
    k = m & np.uint64((1 << (K - 8)) - 1) & np.uint64(0x7FFFFFFF)
    return int(k) if scalar else k


def bucket(key, lgb):
    """bi2_bucket_of: the bucket (of four slots) a key's walk starts in, in a table of 2^lgb buckets"""
    k, scalar = _as_u64(key)
    b = (((k * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - lgb)) & np.uint64((1 << lgb) - 1)
    return int(b) if scalar else b


def table_slots(total):
    """bi2_count_kernel: the table of a bin of `total` records grows 256 -> 512 -> 1024 slots by total + total / 2"""
    n = 256
    while n < SLOTS and n < total + (total >> 1):
        n <<= 1
    return n


def table_lgb(total):
    lgb = 6
    while (4 << lgb) < table_slots(total):
        lgb += 1
    return lgb


def wcap(npos):
    """bigram2_plan: entries of one wave's position list"""
    return (npos * 6 // 10 // WAVES) * 2 + 4096


def region(npos):
    """bigram2_plan over plan_buffers: records one (sub-region, A bin) slot holds — at least: a context's arrays only grow, so one that has held a larger
    corpus keeps larger slots"""
    recs0 = (npos + (npos >> 2)) // BINS * BINS + BINS * SCAT_TILE * 4
    recs1 = max(npos + 1, BINS * SCAT_TILE * 4)
    return 2 * min(recs0, recs1) // (BINS * SUBS)


def pshift(npos):
    """bigram2_plan: position bucket = position >> pshift"""
    s = 12
    while (npos >> s) > 1023:
        s += 1
    return s


# ---- bigrams by final bin ------------------------------------------------------------------------------------------------------------------------------
def keys_in_bin(fbin, n, cb=12, records=0, lo=HEAD, hi=None, in_bucket=None, lgb=None, shuffle=0, avoid=()):
    """n bigrams (a, b), lo <= a, b <= hi, whose final bin is fbin = (A, B) in an order of `records` records. in_bucket / lgb: all of them start their walk
    in that bucket of a table of 2^lgb buckets. shuffle: seed of the order they are drawn in. avoid: bigrams not to return."""
    K = order2_kbits(cb)
    bsh = bshift(records, K)
    free = K - 17 + bsh  # the mix bits the bin does not fix
    assert free <= 22, "too many keys per bin to enumerate"
    hi = (1 << cb) - 1 if hi is None else hi
    y = (np.uint64(fbin[0]) << np.uint64(K - 8)) | (np.uint64(fbin[1]) << np.uint64(free)) | np.arange(1 << free, dtype=np.uint64)
    x = unmix(y, K)
    a, b = x >> np.uint64(cb), x & np.uint64((1 << cb) - 1)
    ok = (a >= lo) & (a <= hi) & (b >= lo) & (b <= hi)
    if in_bucket is not None:
        ok &= bucket(y & np.uint64((1 << (K - 8)) - 1) & np.uint64(0x7FFFFFFF), lgb) == in_bucket
    pairs = list(zip(a[ok].tolist(), b[ok].tolist()))
    np.random.default_rng(shuffle).shuffle(pairs)
    if avoid:
        skip = set(avoid)
        pairs = [p for p in pairs if p not in skip]
    assert len(pairs) >= n, (fbin, n, len(pairs))
    return pairs[:n]


def full_bucket(fbin, lgb, want, cb=12, records=0, lo=HEAD):
    """a bucket of bin fbin's table (2^lgb buckets) that at least `want` bigrams start in, other than the table's last bucket"""
    for bk in range((1 << lgb) // 2, (1 << lgb) - 1):
        try:
            keys_in_bin(fbin, want, cb, records, lo, in_bucket=bk, lgb=lgb)
            return bk
        except AssertionError:
            continue
    raise AssertionError("no bucket with that many keys")


# ---- corpora: one n-gram per sentence ----------------------------------------------------------------------------------------------------------------
class Corpus:
    """items: [(tokens, copies)] — every entry is `copies` sentences of those tokens, in this order (an empty tuple: an empty sentence).
    The builder appends (or, filler_first, prepends) one-token sentences so that every class used occurs at least `mintokens` times — a one-token
    sentence has no window of order 2 — and so that class `top` exists: clsbits is what the test assumes. pad_region: empty sentences are appended until
    one (sub-region, A bin) slot of the order-2 records holds the fullest slot of this corpus (a hot key's records all lie in one A bin)."""

    def __init__(self, items, mintokens=2, top=TOP, closing=True, filler_first=False, pad_region=True, rare=()):
        items = [(tuple(int(t) for t in toks), int(c)) for toks, c in items if c > 0]
        occ = collections.Counter()
        for toks, c in items:
            for t in toks:
                occ[t] += c
        assert all(0 < t <= top for t in occ), "a class beyond the intended range"
        assert all(occ[t] < mintokens for t in rare), "a rare class must not survive order 1"
        filler = [((t,), mintokens - occ[t]) for t in sorted(set(occ) | {top}) if occ[t] < mintokens and t not in rare]
        self.items = filler + items if filler_first else items + filler
        self.mintokens, self.top, self.cb = mintokens, top, clsbits(top)
        self.K = order2_kbits(self.cb)
        self.alive = np.zeros(top + 1, dtype=bool)  # classes that survive order 1
        self.alive[[t for t in set(occ) | {top} if t not in rare]] = True
        sym = self._symbols(self.items)
        if pad_region:
            load = self._slot_load(sym)
            if region(sym.size) < load:  # (beyond the arrays' floor a slot holds one record per 512 positions)
                sym = np.concatenate([sym, np.zeros(BINS * SUBS // 2 * (load + 1) - sym.size, dtype=np.uint32)])
                assert region(sym.size) >= load
        if not closing:
            assert sym[-1] == 0 and sym[-2] != 0
            sym = sym[:-1]
        self.sym = sym
        self.npos = int(sym.size)  # positions: tokens and delimiters
        self.payload = synth.encode_v2(sym).tobytes()
        self._census()

    @staticmethod
    def _symbols(items):
        parts = [np.tile(np.array(toks + (0,), dtype=np.uint32), c) for toks, c in items]
        return np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint32)

    def _windows2(self, sym):
        """positions, left and right class of the admissible windows of order 2: both classes survived order 1 (the delimiter, class 0, never does)"""
        i = np.flatnonzero(self.alive[sym[:-1]] & self.alive[sym[1:]])
        return i, sym[i].astype(np.uint64), sym[i + 1].astype(np.uint64)

    def _slot_load(self, sym):
        i, a, b = self._windows2(sym)
        rec = ~((a < HEAD) & (b < HEAD))
        if not rec.any():
            return 0
        m = mix((a[rec] << np.uint64(self.cb)) | b[rec], self.K)
        sub = ((i[rec] // TILE) % EMIT_GRID) % SUBS  # tile t is emitted by block t mod 512 into sub-region block mod 4
        return int(np.bincount(sub.astype(np.int64) * BINS + (m >> np.uint64(self.K - 8)).astype(np.int64)).max())

    def _census(self):
        i, a, b = self._windows2(self.sym)
        head = (a < HEAD) & (b < HEAD)
        self.head_windows = int(head.sum())
        self.records = int(i.size - self.head_windows)
        self.bshift = bshift(self.records, self.K)
        m = mix((a[~head] << np.uint64(self.cb)) | b[~head], self.K)
        A, B = bin_of_mix(m, self.K, self.bshift)
        fb = (A.astype(np.int64) << 16) | B.astype(np.int64)
        self.bins = {}  # (A, B) -> (records, distinct keys, keys with at least mintokens records)
        for f in np.unique(fb):
            _, cnt = np.unique(m[fb == f], return_counts=True)
            self.bins[(int(f) >> 16, int(f) & 0xFFFF)] = (int(cnt.sum()), int(cnt.size), int((cnt >= self.mintokens).sum()))

    def surviving_windows2(self):
        """positions and position-list shard of the windows of the surviving bigrams outside the head (a bin of the regular walk is counted by a wave of
        queue A & 7, whose list bi2_pospart_kernel sorts into that shard)"""
        i, a, b = self._windows2(self.sym)
        rec = ~((a < HEAD) & (b < HEAD))
        i, m = i[rec], mix((a[rec] << np.uint64(self.cb)) | b[rec], self.K)
        _, inv, cnt = np.unique(m, return_inverse=True, return_counts=True)
        keep = cnt[inv] >= self.mintokens
        return i[keep], ((m[keep] >> np.uint64(self.K - 8)) & np.uint64(7)).astype(np.int64)

    def model(self, maxlength):
        """{key bytes: count} of the patterns train(mintokens, maxlength) keeps, counted window by window from the sentences"""
        cnt = collections.Counter()
        for toks, c in self.items:
            for n in range(1, min(maxlength, len(toks)) + 1):
                for j in range(len(toks) - n + 1):
                    cnt[toks[j:j + n]] += c
        out = {}
        for n in range(1, maxlength + 1):  # (a window with a pruned part occurs no more often than the part: the count alone decides)
            kept = {w: c for w, c in cnt.items() if len(w) == n and c >= self.mintokens}
            if not kept:
                break
            out.update({synth.encode_v2(np.array(w, dtype=np.uint32)).tobytes(): c for w, c in kept.items()})
        return out


def hot_copies_for_wcap(delta, ntok=2, extra_positions=0):
    """copies c of one hot `ntok`-gram, one per sentence, such that c = wcap(positions of that corpus) + delta"""
    for c in range(4000, 5000):
        npos = c * (ntok + 1) + 4 + extra_positions  # (the top class' two one-token sentences)
        if c == wcap(npos) + delta:
            return c
    raise AssertionError("no such count")


# ---- the families of tests/test_gpu_bin_edges.py -------------------------------------------------------------------------------------------------------
class Case:
    """a corpus, the order it is trained to, and what its builder intended: order-2 records, head windows, and the contents of the final bins it is about —
    {(A, B): (records, distinct bigrams, survivors)}. check() holds the corpus (through the restatement above) to these intentions and returns the case."""

    def __init__(self, corpus, records, head=0, bins=None, gives_up=False, note=""):
        self.corpus, self.records, self.head, self.bins, self.gives_up, self.note = corpus, records, head, dict(bins or {}), gives_up, note
        self.reason = 4  # where the case gives up: COLIBRI_FALLBACK_ORDER2 (whatever Bi2State.overflow of order 2 holds — 1 a record slot, 2 a bin's table, 3 a wave's list —,
        # bi2_kept_finish_kernel turns it into DevState.radix_overflow 4)

    def check(self):
        c = self.corpus
        assert (c.records, c.head_windows) == (self.records, self.head), ((c.records, c.head_windows), (self.records, self.head))
        assert c.bshift == 6 and c.cb == 12, "a small order of 12-bit classes: 2048 final bins"
        for f, want in self.bins.items():
            assert c.bins.get(f) == want, (f, c.bins.get(f), want)
        assert region(c.npos) >= c._slot_load(c.sym), "a record slot would overflow"
        return self


A0, B0, C0, D0 = 1000, 2000, 3000, 3500  # the hot n-gram's classes
BIN1, BIN2 = (37, 2), (45, 2)            # two final bins eight apart in the count kernel's walk: the same queue's next bin
ELSEWHERE = (200, 5)


def hot_ngram(n, copies, mintokens=2, wcap_edge=False, pad_region=True):
    """`copies` sentences of one n-gram of classes >= 64: every order's windows of it fill one final bin each. wcap_edge: the case is about the wave's
    position list, which holds wcap(npos) entries — one more window than that and the order gives up. pad_region=False: the corpus stays as small as its
    sentences, and a record slot that cannot hold its share of the hot key's records makes the radix path give up (Bi2State.overflow 1)."""
    toks = (A0, B0, C0, D0)[:n]
    c = Corpus([(toks, copies)], mintokens, pad_region=pad_region)
    if not pad_region:
        return Case(c, (n - 1) * copies, 0, gives_up=region(c.npos) < c._slot_load(c.sym))
    bins = collections.Counter(final_bin(toks[j], toks[j + 1]) for j in range(n - 1))
    return Case(c, (n - 1) * copies, 0, {f: (k * copies, k, k) for f, k in bins.items()}, gives_up=wcap_edge and copies > wcap(c.npos)).check()


def _pick_z(fbins, lefts):
    """a class z such that no bigram (b, z), b in lefts, falls into one of fbins — and (z, z) neither"""
    lefts = np.array(sorted(set(lefts)), dtype=np.uint64)
    for z in range(TOP - 1, HEAD, -1):
        A, B = final_bin(lefts, np.full(lefts.size, z, dtype=np.uint64))
        if not any(((A == f[0]) & (B == f[1])).any() for f in fbins):
            return z
    raise AssertionError("no such class")


def bin_composition(keyed, mintokens=2, with_z=True, elsewhere=True):
    """keyed: {(A, B): [((a, b), copies)]}: the final bins named hold exactly these bigrams, that often. with_z: every sentence is `a b z` with one class z, so
    that every surviving bigram's trigram survives too and a wrong survivor rank or (bin, rank) code shows as merged or missing trigrams; the windows (b, z) fall
    into other bins. elsewhere: one more bigram, mintokens times, in another bin (an order that keeps nothing ends the run)."""
    items, intent = [], {}
    z = _pick_z(list(keyed) + [ELSEWHERE], [b for ks in keyed.values() for (_, b), _ in ks]) if with_z else None
    for f, ks in keyed.items():
        assert len({k for k, _ in ks}) == len(ks)
        items += [(k + ((z,) if with_z else ()), n) for k, n in ks]
        intent[f] = (sum(n for _, n in ks), len(ks), sum(1 for _, n in ks if n >= mintokens))
    nwin = sum(n for ks in keyed.values() for _, n in ks) * (2 if with_z else 1)
    if elsewhere:
        items.append((keys_in_bin(ELSEWHERE, 1)[0], mintokens))
        nwin += mintokens
        intent[ELSEWHERE] = (mintokens, 1, 1)
    order = np.random.default_rng(len(items)).permutation(len(items))  # (the sentences in no particular order: a bin's records arrive mixed)
    return Case(Corpus([items[j] for j in order], mintokens), nwin, 0, intent).check()


def distinct_in_bin(D, second=0):
    """D bigrams, once each, in one final bin (nothing of it survives); second: that many more in the same queue's next bin"""
    keyed = {BIN1: [(k, 1) for k in keys_in_bin(BIN1, D)]}
    if second:
        keyed[BIN2] = [(k, 1) for k in keys_in_bin(BIN2, second)]
    case = bin_composition(keyed, with_z=False)
    case.gives_up = D > MAX_LOAD or second > MAX_LOAD
    return case


def survivors_in_bin(S, D, mintokens=2, low=None):
    """S bigrams `mintokens` times and D - S bigrams `low` times (mintokens - 1 unless given) in one final bin, every sentence `a b z`"""
    low = mintokens - 1 if low is None else low
    keys = keys_in_bin(BIN1, D, shuffle=S)
    return bin_composition({BIN1: [(k, mintokens if j < S else low) for j, k in enumerate(keys)]}, mintokens)


TABLE_TOTALS = {6: 120, 7: 300, 8: 600}  # records of a bin whose table has 2^lgb buckets


def bucket_walk(n, lgb, last):
    """n bigrams that start in ONE bucket of their bin's table — the table's last bucket (the walk wraps to bucket 0) or one in the middle —, survivors and
    singletons alternating, in a bin filled up to the record count that chooses this table size with other bigrams of both kinds"""
    total = TABLE_TOTALS[lgb]
    assert table_lgb(total) == lgb
    bk = (1 << lgb) - 1 if last else full_bucket(BIN1, lgb, 17)
    chain = keys_in_bin(BIN1, n, in_bucket=bk, lgb=lgb)
    ks = [(k, 2 - (j & 1)) for j, k in enumerate(chain)]
    used = sum(c for _, c in ks)
    for j, k in enumerate(keys_in_bin(BIN1, total, avoid=chain, shuffle=n)):
        c = min(2 - (j & 1), total - used)
        if c == 0:
            break
        ks.append((k, c))
        used += c
    case = bin_composition({BIN1: ks})
    case.chain, case.bucket, case.lgb = chain, bk, lgb
    assert case.bins[BIN1][0] == total and all(bucket(inbin_key(a, b), lgb) == bk for a, b in chain)
    return case


HEAD_EDGE = (62, 63, 64, 65)


def head_edge():
    """classes 62 .. 65 in all sixteen ordered pairs. The even pairs survive: once as `x y` and twice as `x y w` (their trigram survives); the odd ones occur
    once, as `x y` or as `x y w` in turn. Exactly the pairs with both classes below 64 are head windows."""
    items, head, total, w = [], 0, 0, 500
    for j, (x, y) in enumerate((x, y) for x in HEAD_EDGE for y in HEAD_EDGE):
        forms = [((x, y), 1), ((x, y, w), 2)] if j % 2 == 0 else [((x, y), 1)] if j % 4 == 1 else [((x, y, w), 1)]
        items += forms
        n = sum(c for _, c in forms)
        total += n + sum(c for t, c in forms if len(t) == 3)  # (the windows (y, w) are records)
        head += n if x < HEAD and y < HEAD else 0
    return Case(Corpus(items), total - head, head).check()


VOCAB = (6, 9, 30, 62, 63, 64, 65, 200, 900, 2500, 4000, 4094)  # some classes below the head's edge, some above


def drawn_sentences(rng, npositions):
    """sentences of 1 .. 12 tokens of VOCAB (frequent classes first), a few of them empty, filling exactly `npositions` positions (delimiters included)"""
    p = 1.0 / np.arange(1, len(VOCAB) + 1)
    out, left = [], npositions
    while left > 0:
        n = 0 if rng.random() < 0.03 else int(rng.integers(1, 13))
        n = min(n, left - 1)
        out.append(tuple(int(t) for t in rng.choice(VOCAB, size=n, p=p / p.sum())))
        left -= n + 1
    return out


_TEXT = []


def aligned_text(s):
    """one drawn text of 9000 positions behind a sentence of s tokens of classes that occur nowhere else (no window of them is admitted): every window of the
    text sits at lane offset (its place + s + 1) mod 64, and the tile and bucket boundaries move through the text with s"""
    if not _TEXT:
        _TEXT.append(drawn_sentences(np.random.default_rng(20260117), 9000))
    prefix = tuple(3000 + j for j in range(s))
    c = Corpus([(prefix, 1)] + [(t, 1) for t in _TEXT[0]], rare=prefix)  # (s = 0: an empty sentence)
    assert c.npos == 9000 + s + 1 + 4
    return Case(c, c.records, c.head_windows).check()


END_NGRAM = (64, 9, 200)


def corpus_end(npos, closing):
    """a drawn text of exactly npos positions that ends in a surviving 3-gram: its last token is the corpus' last token, followed by the closing delimiter or not"""
    rng = np.random.default_rng(npos)
    tail = len(END_NGRAM) + (1 if closing else 0)
    body = [END_NGRAM, END_NGRAM] + drawn_sentences(rng, npos - 4 - 2 * (len(END_NGRAM) + 1) - tail)
    c = Corpus([(t, 1) for t in body] + [(END_NGRAM, 1)], closing=closing, filler_first=True, pad_region=False)
    assert c.npos == npos and c.sym[-1 if not closing else -2] == END_NGRAM[-1]
    return Case(c, c.records, c.head_windows).check()


def list_lengths(k):
    """position bucket 0 holds exactly k windows of surviving bigrams and bucket 1 exactly k + 3; everything else in the two buckets occurs once. The k windows'
    bigrams all belong to one shard (k & 7: the queue of their final bins) and the three more to the next one, so the shard lists of bucket 0 hold k and 0 entries,
    those of bucket 1 k, 3 and 0: every length modulo 4 over the cases."""
    rng = np.random.default_rng(1000 + k)
    s0, s1 = k & 7, (k + 1) & 7

    def in_shard(shard, n, avoid):  # bigrams of bins whose A bin is in that shard's queue, each in a bin of its own
        out = []
        for A in range(shard, 256, 8):
            out += keys_in_bin((A, int(rng.integers(0, 8))), 1, shuffle=k, avoid=avoid + out)
            if len(out) == n:
                return out
        raise AssertionError("not enough bins in that shard")

    def extend(key, shard, avoid):  # a class c such that (key[1], c) belongs to the shard too: `a b c` holds two surviving windows
        for c in rng.permutation(np.arange(HEAD, TOP)).tolist():
            if final_bin(key[1], c)[0] & 7 == shard and (key[1], c) not in avoid and c not in key:
                return key + (c,)
        raise AssertionError("no class extends that bigram within the shard")

    survivors, used = [], []
    for key in in_shard(s0, (k + 1) // 2, []):
        used.append(key)
        if 2 * len(survivors) + 2 <= k:
            key = extend(key, s0, used)
            used.append(key[1:])
        survivors.append(key)
    assert sum(len(t) - 1 for t in survivors) == k
    extra = in_shard(s1, 1, used)[0]
    used.append(extra)

    def singles(npositions):  # sentences `u v` of bigrams that occur once, and one-token sentences, filling exactly that many positions
        out, left = [], npositions
        while left:
            if left in (2, 4):
                out.append((int(rng.integers(HEAD, TOP)),))
                left -= 2
                continue
            u, v = (int(t) for t in rng.integers(HEAD, TOP, size=2))
            if (u, v) not in used:
                used.append((u, v))
                out.append((u, v))
                left -= 3
        return out
    b0 = survivors + singles(TILE - sum(len(t) + 1 for t in survivors))
    b1 = survivors + [extra] * 3
    b1 = b1 + singles(TILE - sum(len(t) + 1 for t in b1))
    c = Corpus([(t, 1) for t in b0 + b1], pad_region=False)
    pos, shard = c.surviving_windows2()
    case = Case(c, c.records, 0).check()
    per = collections.Counter(zip((pos >> 12).tolist(), shard.tolist()))
    assert per == {(0, s0): k, (1, s0): k, (1, s1): 3}, per
    case.lists = per
    return case


def cpu_cases():
    """a few members of every family, small enough for the oracle on the CPU (tests/test_bi2_mix.py): name -> (builder, maxlength)"""
    return {
        "hot_bigram_769": (lambda: hot_ngram(2, 769), 3),
        "hot_bigram_wcap_plus_1": (lambda: hot_ngram(2, hot_copies_for_wcap(1), wcap_edge=True), 2),
        "hot_4gram_4097": (lambda: hot_ngram(4, 4097), 4),
        "distinct_901": (lambda: distinct_in_bin(901), 2),
        "distinct_600_600": (lambda: distinct_in_bin(600, 600), 2),
        "survivors_257_of_300": (lambda: survivors_in_bin(257, 300), 3),
        "survivors_384_of_520": (lambda: survivors_in_bin(384, 520), 3),
        "survivors_257_of_300_min3": (lambda: survivors_in_bin(257, 300, mintokens=3), 3),
        "bucket_walk_17_last_256": (lambda: bucket_walk(17, 6, True), 3),
        "bucket_walk_9_middle_1024": (lambda: bucket_walk(9, 8, False), 3),
        "head_edge": (head_edge, 3),
        "aligned_text_0": (lambda: aligned_text(0), 4),
        "aligned_text_37": (lambda: aligned_text(37), 4),
        "corpus_end_4096_open": (lambda: corpus_end(4096, False), 3),
        "corpus_end_8193_closed": (lambda: corpus_end(8193, True), 3),
        "list_lengths_1": (lambda: list_lengths(1), 3),
        "list_lengths_17": (lambda: list_lengths(17), 3),
    }
