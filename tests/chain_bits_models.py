"""Corpora for tests/test_gpu_chain_bits.py (chain_emit_kernel's successor test: the bucket's bitmap slice in LDS), built on tests/bin_models.py and held to
their intentions on the host (tests/test_chain_step.py runs the builders without a device).

A small corpus has position buckets of 4096 positions (pshift 12). The kernel walks the (position, code) pairs of the surviving (n-1)-grams, list by list —
a list per (bucket, shard), the shard being the count kernel's queue of the (n-1)-gram's final bin; at order 3 a ninth list per bucket holds the windows of the
dense head's class pairs —, in steps of at most 2048 pairs; bucket b is walked by XCD b mod 8, whose blocks take RUN consecutive steps at a time. Window i
becomes a record of order n iff the (n-1)-gram at i + 1 survived too: a bit of the bucket's slice, or of the word behind it when i is the bucket's last position.

edges(last) lays sentences out by position so that all of this occurs, and says so (Edges.check):
  * a surviving (n-1)-gram at a bucket's last position whose successor, the next bucket's first position, survived — and one whose successor did not —, n = 3, 4, 5;
  * the same for head windows of order 2 (both classes below 64): a surviving pair before a surviving one, and a pruned pair before a surviving one;
  * a list longer than a step (one sentence of 4000 equal tokens), with empty buckets on both sides;
  * on some XCD a run of RUN steps that starts in one bucket and ends in another, for RUN = 2, 4, 8; and an XCD with one step;
  * a partial last bucket of `last` positions whose final token ends a surviving 5-gram, the corpus' last position being bit 0 of the bitmap's last word;
    the slice of that bucket is cut at the bitmap's end (ceil(last / 32) + 16 words), those of the others have 129 words: over the cases every count modulo four.
"""
import collections

import numpy as np

import bin_models as bm

BUCKET = 4096   # positions of a bucket at pshift 12
STEP = 2048     # kChStep
XCDS = 8        # kChXcds
SHARDS = 8      # kBi2Shards; list 8 of a bucket: the head windows (order 3)
A, B, C, D, E = 1000, 2000, 3000, 3500, 3600
X = (A, B, C, D, E)      # occurs four times: every n-gram of it survives
U = (101, 102, 103)      # classes that follow a part of X once each
H = (5, 7, 9)            # head classes; occurs three times
HP = (5, 11, 13)         # (5, 11) occurs once, (11, 13) three times
Z, Z2 = 2500, 2600       # the long lists' tokens (a key each: a wave's position list holds ~4100 windows)


def survivors(sym, maxlength, mintokens=2):
    """surv[n][i]: the n-gram at position i lies inside a sentence and occurs at least mintokens times (a window with a pruned part occurs no more often
    than the part: the count alone decides)"""
    surv = {}
    for n in range(1, maxlength + 1):
        m = sym.size - n + 1
        s = np.zeros(sym.size + 1, dtype=bool)
        if m > 0:
            w = np.stack([sym[k:k + m] for k in range(n)], axis=1)
            inside = (w != 0).all(axis=1)
            _, inv, cnt = np.unique(w, axis=0, return_inverse=True, return_counts=True)
            s[:m] = inside & (cnt[inv.ravel()] >= mintokens)
        surv[n] = s
    return surv


class Layout:
    """sentences at chosen positions, empty sentences (one delimiter each) in between"""

    def __init__(self):
        self.items, self.n = [], 0

    def add(self, toks, copies=1):
        self.items.append((tuple(toks), copies))
        self.n += copies * (len(toks) + 1)

    def at(self, pos, toks):
        assert pos >= self.n, (pos, self.n)
        if pos > self.n:
            self.add((), pos - self.n)
        self.add(toks)


class Edges:
    def __init__(self, corpus, last, long):
        self.corpus, self.last, self.long = corpus, last, long
        self.mintokens = corpus.mintokens

    def order3_steps(self):
        """{xcd: [bucket of every step]} of order 3's emit, from the corpus: the lists of order 2's surviving windows outside the head by (bucket, shard), the head
        windows' list of every bucket, each cut into steps, in (bucket, shard) order; and the longest list"""
        c = self.corpus
        pos, shard = c.surviving_windows2()
        lists = collections.Counter(zip((pos // BUCKET).tolist(), shard.tolist()))
        i, a, b = c._windows2(c.sym)
        head = (a < bm.HEAD) & (b < bm.HEAD)
        for bk, k in collections.Counter((i[head] // BUCKET).tolist()).items():
            lists[(bk, SHARDS)] = k
        steps = {x: [] for x in range(XCDS)}
        for (bk, sh), k in sorted(lists.items()):
            steps[bk % XCDS] += [bk] * (-(-k // STEP))
        return steps, max(lists.values()), lists

    def check(self):
        c, sym, npos = self.corpus, self.corpus.sym, self.corpus.npos
        surv = self.surv = survivors(sym, 5, c.mintokens)
        edge = np.arange(BUCKET - 1, npos - 1, BUCKET)
        for n in (3, 4, 5):
            s = surv[n - 1]
            assert (s[edge] & s[edge + 1]).any(), ("no window of order %d admitted across a bucket's end" % n)
            assert (s[edge] & ~s[edge + 1]).any(), ("no window of order %d refused across a bucket's end" % n)
        # head windows of order 2 at a bucket's end: a surviving pair and a pruned one, each before a surviving bigram
        hw = (sym[edge] < bm.HEAD) & (sym[edge + 1] < bm.HEAD) & c.alive[sym[edge]] & c.alive[sym[edge + 1]]
        assert (hw & surv[2][edge] & surv[2][edge + 1]).any() and (hw & ~surv[2][edge] & surv[2][edge + 1]).any()
        # the end: a partial last bucket, the corpus' last token ends a surviving 5-gram, and its position is bit 0 of the bitmap's last word
        assert npos % BUCKET == self.last and (npos - 1) % 32 == 0 and sym[-1] != 0
        assert surv[5][npos - 5] and all(surv[n - 1][npos - n + 1] for n in (3, 4, 5))
        self.slice_words = sorted({min(BUCKET // 32 + 1, (npos + 31) // 32 + 16 - bk * (BUCKET // 32)) for bk in range((npos + BUCKET - 1) // BUCKET)})
        assert self.slice_words == [(self.last + 31) // 32 + 16, 129]
        # steps
        steps, longest, lists = self.order3_steps()
        assert longest == self.long - 1 and (longest > STEP or self.long < STEP), longest
        full = [bk for (bk, sh), k in lists.items() if k > STEP]
        occupied = {bk for bk, _ in lists}
        assert self.long < STEP or any(bk - 1 not in occupied and bk + 1 not in occupied for bk in full), "a full bucket between empty ones"
        for run in (2, 4, 8):
            crossing = [x for x, s in steps.items() for j in range(0, len(s), run) if len(set(s[j:j + run])) > 1]
            assert crossing, ("no run of %d steps crosses a bucket change" % run, steps)
        assert any(len(s) == 1 for s in steps.values()), "an XCD with fewer steps than a run"
        self.steps = steps
        # what the emit kernels admit: windows whose two parts survived
        self.admitted = {n: int((surv[n - 1][:-1] & surv[n - 1][1:]).sum()) for n in (3, 4, 5)}
        self.admitted[2] = c.records + c.head_windows
        return self


def edges(last=577, long=4000):
    """the corpus of the module's docstring; its last bucket holds `last` positions (last - 1 a multiple of 32), its longest sentence `long` tokens (the wide form of
    the chained orders halves a record slot: 1800 equal tokens fit one, 4000 make the run give the chained orders up)"""
    assert (last - 1) % 32 == 0 and 6 <= last < BUCKET
    L = Layout()
    for t in U + (bm.TOP,):  # every class twice: the builder appends nothing, positions are what is written here
        L.add((t,), 2 if t == bm.TOP else 1)
    for t in (X, X, H, H, HP[1:], HP[1:]):
        L.add(t)
    L.add((7, 5))             # a head list of two windows less than the next bucket's ... (the step counts of the buckets differ)
    L.at(1 * BUCKET - 1, X)                 # orders 3, 4, 5: admitted across the edge
    L.at(2 * BUCKET - 1, (A, B, U[0]))      # order 3: (b, u) occurs once
    L.at(3 * BUCKET - 1, (A, B, C, U[1]))   # order 4
    L.at(4 * BUCKET - 1, (A, B, C, D, U[2]))  # order 5
    L.at(5 * BUCKET - 1, H)                 # head windows: (5, 7) survives, and so does (7, 9)
    L.at(6 * BUCKET - 1, HP)                # (5, 11) is pruned, (11, 13) survives
    L.at(7 * BUCKET + 100, (A, B))          # bucket 7, XCD 7: one pair, one step
    L.at(9 * BUCKET, (Z,) * long)           # bucket 9: a list of 3999 windows, two steps; buckets 8, 10 and 11 stay empty
    L.at(12 * BUCKET + 7, (Z2,) * (long * 3 // 4))
    L.at(14 * BUCKET + last - len(X), X)    # ... and the corpus ends with X's last token
    c = bm.Corpus(L.items, closing=False, pad_region=False)
    assert c.items == L.items and c.npos == 14 * BUCKET + last, "the builder added sentences"
    assert bm.pshift(c.npos) == 12
    return Edges(c, last, long).check()
