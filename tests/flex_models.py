"""Models for the flexgram tests, and a vectorised restatement of the abstraction (include/colibri_hip.h: colibri_flexgrams /
colibri_flexgrams_fetch; kernels in csrc/flexgrams.hpp).

restate() says in numpy what colibri_flexgrams_fetch promises — the six arrays, in its layout and in its order — and is itself pinned
to oracle.flexgrams_from_skipgrams by the CPU tests of tests/test_flexgrams.py; tests/test_gpu_flexgrams.py compares the device with it
array for array. The generator builds models in export layout from families whose group structure is known by construction (at token
level, never by scanning bytes), so that a model can be put exactly on a size at which the device code changes path. Nothing here
reads a file; everything is drawn from the numpy Generator the caller hands in.
"""
import collections

import numpy as np

SKIP, FLEX = 3, 4  # the classes of {*} and {**}
Model = collections.namedtuple("Model", "key_off key_bytes ref_off ref_s ref_t")

# a class is written as a varint: 7 bits per byte, low bits first, every byte but the last has its high bit set
VARINT_EDGES = [127, 128, 16383, 16384, (1 << 21) - 1, 1 << 21, (1 << 28) - 1, 1 << 28, (1 << 32) - 1]  # the ends of 1 .. 5 bytes
# classes whose bytes look like a gap: 03 / 04 as the last byte of a longer class, 83 / 84 as an earlier one
GAP_LOOKALIKES = [3 + 3 * 128, 4 + 5 * 128, 5 + 4 * 128, 6 + 3 * 128, 3 + 4 * 128, 4 + 4 * 128, 3 + (3 << 7) + (3 << 14), 4 + (4 << 7) + (4 << 14), 3 + (4 << 7) + (3 << 14)]
VOCAB = VARINT_EDGES + GAP_LOOKALIKES + [6, 7, 100]


def varint(cls):
    out = bytearray()
    while cls >= 128:
        out.append((cls & 127) | 128)
        cls >>= 7
    out.append(cls)
    return bytes(out)


def encode(tokens):
    return b"".join(varint(t) for t in tokens)


def tokens_of(key):
    """the byte strings of a key's tokens (a byte < 128 ends a token)"""
    out, start = [], 0
    for j, b in enumerate(key):
        if b < 128:
            out.append(key[start:j + 1])
            start = j + 1
    return out


def collapse(tokens):
    """token level: every run of {*} becomes one {**}"""
    out = []
    for t in tokens:
        if t != SKIP:
            out.append(t)
        elif not out or out[-1] != FLEX:
            out.append(FLEX)
    return out


def pattern(tokens):
    """(key, key of the flexgram it joins | None) of a token list; the category is decided on the tokens"""
    member = SKIP in tokens and FLEX not in tokens
    return encode(tokens), encode(collapse(tokens)) if member else None


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
def restate(key_off, key_bytes, ref_off, ref_s, ref_t):
    """(fkey_off, fkey_bytes, counts, fref_off, fref_s, fref_t) of a model in export layout, as colibri_flexgrams_fetch writes them:
    every SKIPGRAM (a {*} token, no {**} token; 03 / 04 after a byte >= 128 belong to a longer class) joins the group of its collapsed
    key; groups in ascending order of their lowest member; a group's references = its members' references, ascending by (sentence,
    token), duplicates kept; a group without references is listed with count 0; other categories contribute nothing."""
    ko = np.asarray(key_off).astype(np.int64)
    ro = np.asarray(ref_off).astype(np.int64)
    n = ko.size - 1
    kb = np.asarray(key_bytes, dtype=np.uint8)[: ko[-1]]
    first = np.zeros(kb.size, dtype=bool)  # the first byte of a key
    first[ko[:-1][ko[:-1] < kb.size]] = True
    prevhigh = np.zeros(kb.size, dtype=bool)
    prevhigh[1:] = kb[:-1] >= 128
    prevhigh &= ~first
    gap, flex = ~prevhigh & (kb == SKIP), ~prevhigh & (kb == FLEX)

    def per_key(flag):
        cs = np.concatenate(([0], np.cumsum(flag)))
        return cs[ko[1:]] - cs[ko[:-1]]

    member = (per_key(gap) > 0) & (per_key(flex) == 0)
    again = np.zeros(kb.size, dtype=bool)  # a gap that follows a gap of the same key: dropped
    again[1:] = gap[1:] & gap[:-1]
    again &= ~first
    keep = ~again & np.repeat(member, np.diff(ko))
    collapsed = np.where(gap, np.uint8(FLEX), kb)[keep].tobytes()
    cs = np.concatenate(([0], np.cumsum(keep)))
    members = np.flatnonzero(member)
    group_of = {}  # collapsed key -> group number, in order of first (= lowest) member
    gid = np.fromiter((group_of.setdefault(collapsed[a:b], len(group_of)) for a, b in zip(cs[ko[members]].tolist(), cs[ko[members + 1]].tolist())),
                      dtype=np.int64, count=members.size)
    G = len(group_of)
    fkey_off = np.zeros(G + 1, dtype=np.uint64)
    fkey_off[1:] = np.cumsum(np.fromiter(map(len, group_of), dtype=np.int64, count=G))
    fkey_bytes = np.frombuffer(b"".join(group_of), dtype=np.uint8)
    nref = np.diff(ro)
    group = np.repeat(gid, nref[members])  # the group number of every skipgram reference
    mine = np.repeat(member, nref)
    s = np.asarray(ref_s, dtype=np.uint32)[: ro[-1]][mine]
    t = np.asarray(ref_t, dtype=np.uint16)[: ro[-1]][mine]
    order = np.lexsort((t, s, group))
    counts = np.bincount(group, minlength=G).astype(np.uint32)
    fref_off = np.zeros(G + 1, dtype=np.uint64)
    fref_off[1:] = np.cumsum(counts, dtype=np.uint64)
    return fkey_off, fkey_bytes, counts, fref_off, s[order], t[order]


# ---- families ------------------------------------------------------------------------------------------------------------------------
def singleton(a, b):
    """[a, {*}, b]: a group of its own"""
    return [(encode([a, SKIP, b]), encode([a, FLEX, b]))]


def fanin(a, b, K):
    """[a, {*} x k, b] for k = 1..K: K members of the one group [a, {**}, b]"""
    return [(encode([a] + [SKIP] * k + [b]), encode([a, FLEX, b])) for k in range(1, K + 1)]


def distractors(a, b, c=9):
    """an n-gram, a pattern that already holds a {**}, and the flexgram [a, {**}, b] itself (the key of singleton(a, b) / fanin(a, b, .)): none is a skipgram"""
    return [(encode([a, b]), None), (encode([a, SKIP, c, FLEX, b]), None), (encode([a, FLEX, b]), None)]


def multibyte(rng, n):
    """n distinct short patterns over VOCAB with gaps (and sometimes a {**}) anywhere"""
    seen = {}
    while len(seen) < n:
        toks = [int(rng.choice(VOCAB)) if rng.random() < 0.6 else (SKIP if rng.random() < 0.9 else FLEX) for _ in range(int(rng.integers(2, 7)))]
        k, g = pattern(toks)
        seen.setdefault(k, g)
    return list(seen.items())


def long_keys(rng, n):
    """keys of 100 and more tokens, keys that begin / end with a gap, the key that is gaps only; with their twins of other gap lengths"""
    out = {}
    for j in range(n):
        body = [int(rng.choice(VOCAB)) for _ in range(100 + j)]
        for k in (1, 2, 5):
            for toks in (body[:50] + [SKIP] * k + body[50:], [SKIP] * k + body, body + [SKIP] * k, [SKIP] * k + body[:3] + [SKIP] * (k + 1) + body[3:] + [SKIP] * k):
                out.setdefault(*pattern(toks))
    for k in (1, 2, 3, 120):
        out.setdefault(*pattern([SKIP] * k))
    out.setdefault(*pattern([SKIP, FLEX]))
    return list(out.items())


def singleton_block(n, every=1, first=0):
    """vectorised, for large n: pattern i is [a, {*}, b] where i % every == 0 and the trigram [a, 6, b] otherwise, (a, b) enumerated from pair
    number `first` on (a: two bytes, b: one) -> (n x 4 key matrix, skipgram mask)"""
    i = np.arange(first, first + n, dtype=np.int64)
    assert first + n <= 16256 * 121
    a, b = 128 + i // 121, 7 + i % 121
    isskip = (i - first) % every == 0
    m = np.empty((n, 4), dtype=np.uint8)
    m[:, 0], m[:, 1], m[:, 2], m[:, 3] = (a & 127) | 128, a >> 7, np.where(isskip, SKIP, 6), b
    return m, isskip


# ---- references and assembly ---------------------------------------------------------------------------------------------------------
def draw_refs(rng, n, sentences=(1, 1000)):
    """n references: sentences uniform in the closed range, tokens in 0..65535; in no order"""
    s = rng.integers(sentences[0], sentences[1], size=n, dtype=np.uint64, endpoint=True).astype(np.uint32)
    t = rng.integers(0, 65536, size=n, dtype=np.uint32).astype(np.uint16)
    return s, t


def assemble(keys, counts, ref_s, ref_t, perm=None):
    """the five arrays of export layout. keys: a list of bytes or an (n, w) uint8 matrix; counts: references per pattern; ref_s / ref_t: all
    references, pattern after pattern in the order of `keys`; perm: the model's pattern j is keys[perm[j]] (with its references)"""
    counts = np.asarray(counts, dtype=np.int64)
    n = counts.size
    perm = np.arange(n) if perm is None else np.asarray(perm)
    if isinstance(keys, np.ndarray):
        lens, key_bytes = np.full(n, keys.shape[1], dtype=np.int64), np.ascontiguousarray(keys[perm]).reshape(-1)
    else:
        keys = [keys[i] for i in perm.tolist()]
        lens, key_bytes = np.fromiter(map(len, keys), dtype=np.int64, count=n), np.frombuffer(b"".join(keys), dtype=np.uint8)
    key_off, ref_off, old_off = np.zeros(n + 1, dtype=np.uint64), np.zeros(n + 1, dtype=np.uint64), np.zeros(n + 1, dtype=np.int64)
    key_off[1:] = np.cumsum(lens)
    old_off[1:] = np.cumsum(counts)
    ref_off[1:] = np.cumsum(counts[perm])
    src = np.repeat(old_off[:-1][perm] - ref_off[:-1].astype(np.int64), counts[perm]) + np.arange(int(old_off[-1]))
    return Model(key_off, key_bytes, ref_off, np.asarray(ref_s, dtype=np.uint32)[src], np.asarray(ref_t, dtype=np.uint16)[src])


def build(rng, pats, counts, sentences=(1, 1000), shuffle=True, refs=None, plant=True):
    """pats: [(key, group key | None)] from the families; counts: references per pattern -> (Model, groups). The references are drawn
    (draw_refs) unless refs = (sentences, tokens) gives them, flat and in the order of pats. plant: every member with two references holds
    one exact duplicate, and in every group each member with references repeats one reference of the member before it. The patterns are
    then shuffled. groups = [(group key, ascending member numbers)] in ascending order of the lowest member: the structure as constructed,
    in the model's numbering."""
    counts = np.asarray(counts, dtype=np.int64)
    n = len(pats)
    assert counts.size == n and len({k for k, _ in pats}) == n
    off = np.concatenate(([0], np.cumsum(counts)))
    s, t = draw_refs(rng, int(off[-1]), sentences) if refs is None else (np.array(refs[0], dtype=np.uint32), np.array(refs[1], dtype=np.uint16))
    by_group = {}
    for i, (_, g) in enumerate(pats):
        if g is not None:
            by_group.setdefault(g, []).append(i)
    if plant:
        for members in by_group.values():
            have = [i for i in members if counts[i]]
            for a, b in zip(have, have[1:]):
                s[off[b]], t[off[b]] = s[off[a]], t[off[a]]
            for i in have:
                if counts[i] >= 2:
                    s[off[i + 1] - 1], t[off[i + 1] - 1] = s[off[i]], t[off[i]]
    perm = rng.permutation(n) if shuffle else np.arange(n)
    number = np.empty(n, dtype=np.int64)
    number[perm] = np.arange(n)
    groups = sorted(((g, sorted(number[m].tolist())) for g, m in by_group.items()), key=lambda x: x[1][0])
    return assemble([k for k, _ in pats], counts, s, t, perm), groups


def family_model(rng, npatterns, sentences=(1, 1000), maxrefs=6):
    """a small model of every family, about npatterns patterns: singletons, fan-in groups of 2..9 members, their distractors, multi-byte and
    long keys; 0..maxrefs references per pattern (a fifth of the patterns have none)"""
    words = [int(w) for w in rng.permutation(VOCAB + list(range(8, 40)))]
    pats = {}
    pairs = [(a, b) for a in words for b in words]
    order = rng.permutation(len(pairs))
    j = 0
    while len(pats) < npatterns * 6 // 10:
        a, b = pairs[order[j]]
        j += 1
        kind = rng.integers(0, 4)
        new = singleton(a, b) if kind == 0 else fanin(a, b, int(rng.integers(2, 10))) if kind == 1 else singleton(a, b) + distractors(a, b) if kind == 2 else fanin(a, b, 3) + distractors(a, b)
        for k, g in new:
            pats.setdefault(k, g)
    for k, g in long_keys(rng, 2) + multibyte(rng, max(0, npatterns - len(pats) - 40)):
        pats.setdefault(k, g)
    pats = list(pats.items())
    counts = rng.integers(0, maxrefs + 1, size=len(pats)) * (rng.random(len(pats)) >= 0.2)
    members = collections.defaultdict(list)
    for i, (_, g) in enumerate(pats):
        members[g].append(i)
    counts[next(m for g, m in members.items() if g is not None and len(m) > 1)] = 0  # one group of several members, none with a reference
    return build(rng, pats, counts, sentences)
