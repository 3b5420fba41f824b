"""Pattern relations on the device (colibri_relations / colibri_relations_resident; colibri-patternmodeller --subsumes / --subsumed /
--leftneighbours / --rightneighbours), against the reference's per-pattern functions (tests/golden/relations/) and the restatement in
test_relations.py."""
import os
import random
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN
from test_cooc import CLI, COOC, MODELS, key_tokens, load_model, reverse_index, sentences
from test_gpu_cooc import flat
from test_oracle import read_payload
from test_relations import FUNCTIONS, KINDS, THRESHOLDS, load_fixture, related

pytestmark = pytest.mark.gpu


def rows_of(keys, a, b, c):
    return [((keys[x], keys[y]), int(z)) for x, y, z in zip(a.tolist(), b.tolist(), c.tolist())]


def check_order(rows, number):
    """by A's pattern number, then count descending, then B's key bytes"""
    for ((a0, b0), c0), ((a1, b1), c1) in zip(rows, rows[1:]):
        assert (number[a0], -c0, b0) < (number[a1], -c1, b1), (a0, b0, c0, a1, b1, c1)


def device_relations(ctx, counts, refs, payload, fn, thr=0):
    keys, key_off, kb, ref_off, rs, rt = flat(counts, refs)
    ctx.upload(payload)
    rows = rows_of(keys, *ctx.relations(key_off, kb, ref_off, rs, rt, KINDS[fn], threshold=thr))
    check_order(rows, {k: j for j, k in enumerate(keys)})
    return rows


@pytest.fixture(scope="module")
def ctx():
    from colibri_amd import capi
    with capi.Context(0) as c:
        yield c


@pytest.mark.parametrize("thr", THRESHOLDS)
@pytest.mark.parametrize("corpus,kind", MODELS)
def test_loaded_model_matches_the_reference(ctx, corpus, kind, thr):
    counts, refs = load_model(corpus, kind)
    payload = read_payload(corpus)
    for fn in FUNCTIONS:
        rows = device_relations(ctx, counts, refs, payload, fn, thr)
        want = load_fixture(fn, corpus, kind, thr)
        assert dict(rows) == want and len(rows) == len(want), fn


def exported(ctx):
    key_off, key_bytes, counts, (ref_off, rs, rt) = ctx.export_arrays()
    kb, off = key_bytes.tobytes(), key_off.tolist()
    keys = [kb[off[j]:off[j + 1]] for j in range(len(counts))]
    cnt = {k: int(c) for k, c in zip(keys, counts.tolist())}
    refs = {k: list(zip(rs[int(ref_off[j]):int(ref_off[j + 1])].tolist(), rt[int(ref_off[j]):int(ref_off[j + 1])].tolist())) for j, k in enumerate(keys)}
    return keys, cnt, refs


@pytest.mark.parametrize("corpus,kind", MODELS)
def test_resident_model_matches_the_reference(ctx, corpus, kind):
    """the model trained on the device with the fixtures' options (tests/golden/relations/README.md) is the reference's; its resident relations
    are the reference's rows"""
    payload = read_payload(corpus)
    ctx.upload(payload)
    small = corpus in ("hamlet.v2", "edge")
    ctx.train(mintokens=2 if small else 15, maxlength=4 if small else 3, indexed=1, doskipgrams=kind == "is", minskiptypes=2)
    keys, cnt, refs = exported(ctx)
    assert cnt == load_model(corpus, kind)[0]
    number = {k: j for j, k in enumerate(keys)}
    for thr in THRESHOLDS:
        for fn in FUNCTIONS:
            rows = rows_of(keys, *ctx.relations_resident(KINDS[fn], threshold=thr))
            check_order(rows, number)
            assert dict(rows) == load_fixture(fn, corpus, kind, thr), (fn, thr)


@pytest.mark.parametrize("corpus,kind", [("hamlet.v2", "is"), ("edge", "is")])
def test_forced_small_chunks_give_the_same_rows(ctx, corpus, kind, monkeypatch):
    """COLIBRI_REL_CHUNK of 1 / 5 / 7 events: chunks cut inside patterns, the runs of a cut pattern carried and merged before the threshold;
    the rows are those of one chunk, in the same order"""
    counts, refs = load_model(corpus, kind)
    payload = read_payload(corpus)
    for fn in FUNCTIONS:
        for thr in THRESHOLDS:
            one = device_relations(ctx, counts, refs, payload, fn, thr)
            events1, chunks1, scratch1 = ctx.relations_info()
            assert chunks1 == 1 and events1 >= sum(c for _, c in one)
            for budget in ("1", "5", "7"):
                monkeypatch.setenv("COLIBRI_REL_CHUNK", budget)
                many = device_relations(ctx, counts, refs, payload, fn, thr)
                events, chunks, scratch = ctx.relations_info()
                monkeypatch.delenv("COLIBRI_REL_CHUNK")
                assert events == events1 and chunks >= events // int(budget)
                assert many == one, (fn, thr, budget)


def relations_of(fn, counts, refs, payload, picked, thr):
    """the restatement for the patterns `picked` only, by position (the reverse index of the sentences they occur in)"""
    sents = sentences(payload)
    need = sorted({s for a in picked for s, _ in refs[a]})
    at_pos = {}
    for s, occ in zip(need, reverse_index(counts, [sents[s - 1] for s in need])):
        d = at_pos[s - 1] = {}
        for i, n, b in occ:
            d.setdefault(i, []).append((n, b))
    maxn = max(len(key_tokens(k)) for k in counts)
    out = {}
    for a in picked:
        at = key_tokens(a)
        na = len(at)
        rel = {}
        for s, t in refs[a]:
            toks, d = sents[s - 1], at_pos[s - 1]
            for i in range(max(0, t - maxn), t + na + 1):
                for n, b in d.get(i, ()):
                    if thr and counts[b] < thr:
                        continue
                    if related(fn, a, at, t, i, b, toks[i:i + n], toks):
                        rel[b] = rel.get(b, 0) + 1
        out.update({(a, b): c for b, c in rel.items() if thr == 0 or c >= thr})
    return out


@pytest.mark.parametrize("phrases", [False, True])
def test_a_million_tokens_with_skipgrams_against_the_restatement(ctx, phrases):
    from colibri_amd import synth
    payload = synth.zipf_corpus(1_000_000, 3000, 11, phrases=phrases, header=False)
    ctx.upload(payload)
    ctx.train(mintokens=20, maxlength=3, indexed=1, doskipgrams=True, minskiptypes=2)
    keys, cnt, refs = exported(ctx)
    assert any(b"\x03" in key_tokens(k) for k in keys)
    rnd = random.Random(5)
    skips = [k for k in keys if b"\x03" in key_tokens(k)]
    picked = set(rnd.sample([k for k in keys if cnt[k] <= 2000], 150)) | set(rnd.sample(skips, min(50, len(skips))))
    for fn in FUNCTIONS:
        for thr in (0, 25):
            got = {k: c for k, c in rows_of(keys, *ctx.relations_resident(KINDS[fn], threshold=thr)) if k[0] in picked}
            assert got == relations_of(fn, cnt, refs, payload, picked, thr), (fn, thr)


def test_ten_million_tokens_ngram_invariants(ctx):
    """n-grams only: the forward index holds every occurrence of every pattern, so right(A)[B] = left(B)[A], subchildren(A)[B] = subparents(B)[A],
    and the right-neighbour counts sum to the adjacent occurrence pairs, counted here from the forward index alone"""
    from colibri_amd import synth
    payload = synth.zipf_corpus(10_000_000, 20000, 3, phrases=True, header=False)
    ctx.upload(payload)
    ctx.train(mintokens=2, maxlength=4, indexed=1)
    key_off, key_bytes, counts, (ref_off, rs, rt) = ctx.export_arrays()
    npat = len(counts)

    def pairs(kind, swap=False):
        a, b, c = ctx.relations_resident(kind)
        a, b = (b, a) if swap else (a, b)
        code = a.astype(np.uint64) * np.uint64(npat) + b.astype(np.uint64)
        order = np.argsort(code, kind="stable")
        return code[order], c[order]

    left, right = pairs(2), pairs(3, swap=True)  # left(A)[B] against right(B)[A] (kinds: 2 = getleftneighbours, 3 = getrightneighbours)
    assert len(right[0]) > 10 ** 5
    assert np.array_equal(right[0], left[0]) and np.array_equal(right[1], left[1])
    kids, parents = pairs(0), pairs(1, swap=True)
    assert len(kids[0]) > 10 ** 5
    assert np.array_equal(kids[0], parents[0]) and np.array_equal(kids[1], parents[1])
    # adjacent pairs: A at (s, t), any pattern starting at (s, t + n(A)) — the forward index holds every one of them
    kb = np.frombuffer(key_bytes.tobytes(), dtype=np.uint8)
    ntok = np.add.reduceat((kb < 128).astype(np.int64), key_off[:-1].astype(np.int64))
    ntok[np.diff(key_off.astype(np.int64)) == 0] = 0
    per = np.diff(ref_off.astype(np.int64))
    n_of_ref = np.repeat(ntok, per)
    pos = (rs.astype(np.int64) << 16) | rt.astype(np.int64)
    starts = np.bincount(np.searchsorted(np.unique(pos), pos), minlength=len(np.unique(pos)))
    upos = np.unique(pos)
    nxt = pos + n_of_ref
    at = np.searchsorted(upos, nxt)
    hit = (at < len(upos)) & (upos[np.minimum(at, len(upos) - 1)] == nxt)
    adjacent = int(starts[at[hit]].sum())
    assert int(right[1].astype(np.int64).sum()) == adjacent


def _blocks(text, label):
    """the CLI's relation output: [(pattern line, [(count, frequency, count2)] in printed order)], the header's line number (two patterns may
    print as the same text, so blocks are kept in order, not by their text)"""
    blocks, header_at = [], None
    for j, ln in enumerate(text.splitlines()):
        if ln.startswith("#\t"):
            assert ln == "#\tPATTERN1\tRELATION\tPATTERN2\tREL.COUNT\tREL.FREQUENCY\tCOUNT2"
            header_at = j
        elif ln.startswith("\t"):
            f = ln.split("\t")
            assert f[1] == blocks[-1][0] and f[2] == label
            blocks[-1][1].append((int(f[4]), f[5], int(f[6])))
        else:
            blocks.append((ln, []))
    return blocks, header_at


@pytest.mark.parametrize("corpus,kind", [("hamlet.v2", "is"), ("edge", "is"), ("zipf20k", "i")])
def test_cli_relation_flags_against_the_reference(corpus, kind):
    data = os.path.join(GOLDEN, corpus + ".colibri.dat")
    cls = os.path.join(GOLDEN, "hamlet.colibri.cls" if corpus.startswith("hamlet") else "synthetic.colibri.cls")
    model = os.path.join(COOC, f"{corpus}.{kind}.colibri.patternmodel")
    counts, _ = load_model(corpus, kind)
    for flag, fn, label in (("--subsumes", "getsubchildren", "SUBSUMES"), ("--subsumed", "getsubparents", "SUBSUMED-BY"),
                            ("--leftneighbours", "getrightneighbours", "LEFT-NEIGHBOUR-OF"), ("--rightneighbours", "getleftneighbours", "RIGHT-NEIGHBOUR-OF")):
        out = subprocess.run([CLI, "-i", model, "-f", data, "-c", cls, flag], capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        blocks, header_at = _blocks(out.stdout, label)
        assert len(blocks) == len(counts) and header_at == 1
        for _, rows in blocks:
            assert [c for c, _, _ in rows] == sorted((c for c, _, _ in rows), reverse=True)
        want = {}
        for (a, b), c in load_fixture(fn, corpus, kind, 0).items():
            want.setdefault(a, []).append((c, counts[b]))
        want_blocks = []
        for a, rs in want.items():
            total = sum(c for c, _ in rs)
            want_blocks.append(sorted((c, f"{c / total:.6g}", c2) for c, c2 in rs))
        got_blocks = [sorted(r) for _, r in blocks if r]
        assert sorted(got_blocks) == sorted(want_blocks)
