"""Skipgrams of a loaded indexed model on the device (csrc/modelskip.hpp behind colibri_modelskip / colibri_modelskip_resident /
colibri_modelskip_fetch / colibri_modelskip_info) against the plain restatement tests/modelskip_models.py::restate, which
tests/test_modelskip.py pins to the fixtures the reserved reference left and to the direct -s builds: the kept skipgrams with their counts,
skip-type counts and reference lists (exact and ascending), the keep bytes against the restatement's erased set, the per-order figures; then
the C++ face and the CLI on the same fixtures.

ONE context serves the device tests, large and tiny models in turn: that a context may be used again is part of what is tested."""
import copy
import gzip
import os
import shutil
import subprocess

import numpy as np
import pytest

import modelskip_models as mm
from conftest import GOLDEN
from test_oracle import read_payload

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "colibri-core_amd", "bin")
CLI = os.path.join(BIN, "colibri-patternmodeller")


@pytest.fixture(scope="module")
def ctx():
    from colibri_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def check(ctx, model, opts, order=None, tag=None):
    """the device's answer on `model` installed in a copy of it == the restatement on another copy; returns (the restated model, its log, its trace)"""
    arrays = mm.to_arrays(model, order)
    keys = arrays[5]
    answer = ctx.model_skipgrams(*arrays[:5], **opts)
    trace = {}
    want = copy.deepcopy(model)
    log, has, types = mm.restate(want, trace=trace, **opts)
    compare(ctx, model, keys, answer, want, log, types, trace, tag)
    return want, log, trace


def compare(ctx, model, keys, answer, want, log, types, trace, tag=None):
    rows, keep = mm.answer_rows(answer)
    for k, cnt, ty, refs in rows:
        assert refs == sorted(refs) and cnt == len(refs), (tag, k)  # ascending (sentence, token), the count is the list's length
        assert types[k] == ty, (tag, k, ty, types[k])
    assert len({r[0] for r in rows}) == len(rows), tag
    assert [len(r[0]) for r in rows] == sorted(len(r[0]) for r in rows), tag  # by order
    assert [k for k, flag in zip(keys, keep) if not flag] == [k for k in keys if k not in want], tag  # the erased set
    got = mm.apply_answer(model, keys, answer)
    assert got == want, (tag, sorted(set(got) ^ set(want))[:5], [k for k in got if k in want and got[k] != want[k]][:3])
    info, candidates, scratch = ctx.model_skipgrams_info()
    assert [list(r) for r in info] == log, (tag, info, log)
    assert candidates == trace["candidates"], tag
    assert ctx.modelskip_erased == sum(1 for k in keys if k not in want), tag
    assert scratch > 0 or not keys, tag


# ---- the fixtures of the reserved reference and the direct builds, uploaded ----------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(mm.cases()))
def test_fixtures_uploaded(ctx, name):
    c, model, want, _ = mm.fixture(name)
    got, log, _ = check(ctx, model, mm.case_options(c), tag=name)
    assert got == want and log == c["orders"]


@pytest.mark.parametrize("igold,isgold,opts", mm.DIRECT, ids=[d[1] for d in mm.DIRECT])
def test_direct_builds_uploaded(ctx, igold, isgold, opts):
    model, want = mm.direct_pair(igold, isgold)
    got, _, _ = check(ctx, model, opts, tag=isgold)
    assert got == want


# ---- the resident form: a colibri_train without skipgrams, then the skipgrams of the model where it lies ----------------------------------------------
@pytest.mark.parametrize("corpus,isgold,T", [("hamlet.v2", "hamlet.v2.is.l5.txt", 2), ("hamlet.v2", "hamlet.v2.isT1.l5.txt", 1), ("zipf20k", "zipf20k.is.l5.txt", 2),
                                              ("phrases15k", "phrases15k.isT1.l5.txt", 1)])
def test_resident_equals_uploaded_and_the_direct_build(ctx, corpus, isgold, T):
    want = mm.load_rows(os.path.join(GOLDEN, isgold))
    ctx.upload(read_payload(corpus))
    ctx.train(mintokens=2, maxlength=5, indexed=1)
    before = ctx.export_arrays()
    opts = dict(mintokens=2, minskiptypes=T, maxlength=5)
    resident = ctx.model_skipgrams(resident=True, **opts)
    info_resident = ctx.model_skipgrams_info()[0]
    key_off, key_bytes, _, (ref_off, rs, rt) = before
    uploaded = ctx.model_skipgrams(key_off, key_bytes, ref_off, rs, rt, **opts)
    assert ctx.model_skipgrams_info()[0] == info_resident
    for a, b in zip(resident[:4] + resident[4] + (resident[5],), uploaded[:4] + uploaded[4] + (uploaded[5],)):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    kb, off, ro = key_bytes.tobytes(), key_off.tolist(), ref_off.tolist()
    s, t = rs.tolist(), rt.tolist()
    keys = [mm.tokens_of(kb[off[j]:off[j + 1]]) for j in range(len(off) - 1)]
    model = {k: list(zip(s[ro[j]:ro[j + 1]], t[ro[j]:ro[j + 1]])) for j, k in enumerate(keys)}
    assert mm.apply_answer(model, keys, resident) == want
    after = ctx.export_arrays()  # the context's own model is as it was
    for a, b in zip(before[:3] + before[3], after[:3] + after[3]):
        assert np.array_equal(a, b)


# ---- a crafted model -----------------------------------------------------------------------------------------------------------------------------
W = [mm.varint(5), mm.varint(200), mm.varint(20000), mm.varint(3000000)]  # class ids of 1, 2, 3 and 4 bytes
assert [len(w) for w in W] == [1, 2, 3, 4]


class Crafted:
    """patterns with fresh references each; close(k) also gives every contiguous part of k that the model lacks"""

    def __init__(self):
        self.model, self.next = {}, 0

    def tok(self):
        self.next += 1
        return mm.varint(1000 + 37 * self.next)  # two and three bytes, never 03 / 04, never one of W

    def refs(self, n):
        out = [(1 + (self.next * 7919 + i * 104729) % 60000, (self.next + 3 * i) % 65536) for i in range(n)]
        self.next += 1
        assert len(set(out)) == n
        return out

    def add(self, k, count):
        k = tuple(k)
        if k not in self.model:
            self.model[k] = self.refs(count)
        return k

    def close(self, k, count, parts=2):
        k = tuple(k)
        for n in range(1, len(k)):
            for i in range(len(k) - n + 1):
                self.add(k[i:i + n], parts)
        return self.add(k, count)


def crafted_model():
    c = Crafted()
    a, b, x, y, z = (c.tok() for _ in range(5))
    named = {"width": []}
    # a masked token of each byte width at the first and at the last inner position, orders 3 to 6; two sources per shape so that T = 2 keeps some
    for n in (3, 4, 5, 6):
        for w in W:
            for other in (x, y):
                inner_first = (a, w) + (other,) * (n - 3) + (b,)
                inner_last = (a,) + (other,) * (n - 3) + (w, b)
                named["width"] += [(c.close(inner_first, 2), 1), (c.close(inner_last, 2), n - 2)]
    # groups of exactly 1, 2, 3 and 4 sources with a reference each: T - 1 and T for T = 2, 3, 4; counts t - 1 and t for t = 2, 3, 4
    l, r = c.tok(), c.tok()
    for members in (1, 2, 3, 4):
        l2 = c.tok()
        for _ in range(members):
            c.close((l, l2, c.tok(), r), 1, parts=4)
        named["members%d" % members] = (l, l2, mm.GAP, r)
    # an n-gram missing only its left slice, one missing only its right
    p, q, s = c.tok(), c.tok(), c.tok()
    c.add((p,), 3), c.add((q,), 3), c.add((s,), 3)
    c.add((q, s), 3)
    named["no_left"] = c.add((p, q, s), 3)
    p2, q2, s2 = c.tok(), c.tok(), c.tok()
    c.add((p2, q2), 3)
    named["no_right"] = c.add((p2, q2, s2), 3)
    # an order-3 n-gram below t = 2 whose erasure invalidates an order-4 n-gram that is itself frequent
    g = (c.tok(), c.tok(), c.tok())
    c.close(g, 1, parts=5)
    named["weak3"] = g
    named["orphan4"] = c.close(g + (c.tok(),), 5, parts=5)
    # one hot group of 300 sources: more than a block's lanes
    h1, h2 = c.tok(), c.tok()
    for i in range(300):
        c.close((h1, mm.varint(2000000 + i), h2), 1 + i % 3)
    named["hot"] = (h1, mm.GAP, h2)
    # one source list of 5000 references, sentence numbers up to 2^32 - 2
    big = c.close((c.tok(), c.tok(), c.tok()), 2)
    top = 2 ** 32 - 2
    sent = sorted({top, top - 1, 0, 1, 255, 256, 65535, 65536, 2 ** 24 - 1, 2 ** 24} | {(i * 858993) % top for i in range(5000)})[-5000:]
    c.model[big] = [(s_, (i * 13) % 65536) for i, s_ in enumerate(sent)]
    assert len(c.model[big]) == 5000 and c.model[big][-1][0] == top
    named["big"] = big
    return c.model, named


@pytest.fixture(scope="module")
def crafted():
    return crafted_model()


def shuffled(model, seed):
    keys = sorted(model, key=lambda k: b"".join(k))
    return [keys[i] for i in np.random.default_rng(seed).permutation(len(keys))]


@pytest.mark.parametrize("t,T,maxskips", [(2, 2, 3), (2, 1, 3), (3, 3, 2), (4, 4, 1), (1, 1, 3), (2, 3, 1)])
def test_crafted_model(ctx, crafted, t, T, maxskips):
    model, named = crafted
    assert 500 < len(model) < 4000
    got, log, trace = check(ctx, model, dict(mintokens=t, minskiptypes=T, maxlength=6, maxskips=maxskips), order=shuffled(model, 7 * t + T), tag=(t, T, maxskips))
    groups = trace["groups"]
    if t <= 2:  # (a higher t erases this family's 3-grams, of two references each, and with them the longer members' slices)
        assert [r[0] for r in log] == [3, 4, 5, 6] and all(r[1] for r in log)
        # every byte width was masked at the first and at the last inner position, at every order
        assert {(len(src), len(src[pos]), pos == 1) for src, pos in named["width"]} == {(n, w, f) for n in (3, 4, 5, 6) for w in (1, 2, 3, 4) for f in (False, True) if f or n > 3}
        for src, pos in named["width"]:
            assert src not in trace["invalid"] and src[:pos] + (mm.GAP,) + src[pos + 1:] in groups
        # the masks: at n = 5 `0b01010` has two gaps and goes when maxskips = 1; the candidates the device counted are the restatement's (compare)
        assert len(mm.gap_masks(5, maxskips)) == (6 if maxskips == 1 else 7)
        assert any(len(k) == 5 and k[1] == mm.GAP and k[3] == mm.GAP and k[2] != mm.GAP for k in groups) == (maxskips != 1)
    # groups of exactly T - 1 and T sources, counts of exactly t - 1 and t
    for m in (1, 2, 3, 4):
        assert groups[named["members%d" % m]] == (m, m)
        assert (named["members%d" % m] in got) == (m >= t and (T <= 1 or m >= T))
    # the slices
    if t > 1:
        assert named["no_left"] in trace["invalid"] and named["no_right"] in trace["invalid"]
        assert named["orphan4"] in trace["invalid"] and named["weak3"] not in got and named["orphan4"] in got
    else:
        assert not trace["invalid"] and named["weak3"] in got
    assert groups[named["hot"]] == (sum(1 + i % 3 for i in range(300)), 300) and named["hot"] in got
    bigskip = (named["big"][0], mm.GAP, named["big"][2])
    assert (bigskip in got) == (T <= 1) and groups[bigskip] == (5000, 1)
    if T <= 1:
        assert got[bigskip][-1][0] == 2 ** 32 - 2


def test_order_with_nothing_found_is_left_unpruned(ctx):
    """every 4-gram misses a slice: the loop ends at order 4 before its prune, and the 4- and 5-grams below t stay"""
    c = Crafted()
    for _ in range(5):
        c.close((c.tok(), c.tok(), c.tok()), 2)
    weak3 = c.close((c.tok(), c.tok(), c.tok()), 1)
    four = [c.add((c.tok(), c.tok(), c.tok(), c.tok()), 1) for _ in range(3)]
    five = [c.add((c.tok(),) * 5, 1)]
    got, log, _ = check(ctx, c.model, dict(mintokens=2, minskiptypes=1, maxlength=6), order=shuffled(c.model, 3))
    assert log == [[3, 6, 2, 0], [4, 0, 0, 0]]  # the weak 3-gram and its skipgram go
    assert weak3 not in got and all(k in got for k in four + five)


def test_empty_model_and_a_model_without_three_tokens(ctx):
    answer = ctx.model_skipgrams(np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint16))
    rows, keep = mm.answer_rows(answer)
    assert rows == [] and keep == [] and ctx.model_skipgrams_info()[0] == [(3, 0, 0, 0)]  # `Counting 3-skipgrams`, ` None found`
    c = Crafted()
    for _ in range(4):
        c.close((c.tok(), c.tok()), 3)
    got, log, _ = check(ctx, c.model, dict(mintokens=2, minskiptypes=1, maxlength=5))
    assert got == c.model and log == [[3, 0, 0, 0]]


# ---- the group hash of a few bits: the byte compares decide, the retries run ------------------------------------------------------------------------
def test_hash_bits_hook(ctx, crafted, monkeypatch):
    from colibri_amd import capi
    model, _ = crafted
    opts = dict(mintokens=2, minskiptypes=2, maxlength=6)
    check(ctx, model, opts, tag="no switch")
    monkeypatch.setenv("COLIBRI_MSKIP_HASH_BITS", "3")  # the first three seeds collide, the fourth decides
    check(ctx, model, opts, tag="3")
    monkeypatch.setenv("COLIBRI_MSKIP_HASH_BITS", "3:2")  # two retries
    check(ctx, model, opts, tag="3:2")
    monkeypatch.setenv("COLIBRI_MSKIP_HASH_BITS", "3:4")
    with pytest.raises(capi.ColibriError) as e:
        ctx.model_skipgrams(*mm.to_arrays(model)[:5], **opts)
    assert e.value.code == capi.ERR_OVERFLOW and "collision" in str(e.value)
    monkeypatch.delenv("COLIBRI_MSKIP_HASH_BITS")
    check(ctx, model, opts, tag="switch off again")


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["skipgram", "flexgram", "32 tokens"])
def test_refusals(ctx, what):
    from colibri_amd import capi
    c = Crafted()
    c.close((c.tok(), c.tok(), c.tok()), 2)
    if what == "skipgram":
        c.add((c.tok(), mm.GAP, c.tok()), 2)
    elif what == "flexgram":
        c.add((c.tok(), mm.FLEX, c.tok()), 2)
    else:
        c.add(tuple(c.tok() for _ in range(32)), 2)
    with pytest.raises(capi.ColibriError) as e:
        ctx.model_skipgrams(*mm.to_arrays(c.model)[:5], mintokens=2, minskiptypes=1, maxlength=100)
    assert e.value.code == capi.ERR_UNSUPPORTED
    assert ("32 tokens" if what == "32 tokens" else what + "s") in str(e.value)
    if what == "32 tokens":  # below the long key's order nothing is wrong
        check(ctx, c.model, dict(mintokens=2, minskiptypes=1, maxlength=31))


# ---- the CLI: -i <indexed model of n-grams> [-f corpus] -s ------------------------------------------------------------------------------------------
def model_file(name, tmp_path):
    """a fixture model as a file the CLI can read (the large ones are stored gzipped)"""
    path = os.path.join(mm.FIXTURES, name)
    if not name.endswith(".gz"):
        return path
    out = str(tmp_path / name[:-3])
    with gzip.open(path, "rb") as f, open(out, "wb") as g:
        shutil.copyfileobj(f, g)
    return out


def cli_options(c):
    args = ["-l", str(c["l"]), "-T", str(c["T"])]
    return args + (["-t", str(c["t"])] if c["t"] != -1 else [])


def in_order(lines, text):
    """the lines as one contiguous block of the text's lines"""
    have = text.splitlines()
    return any(have[i:i + len(lines)] == lines for i in range(len(have) - len(lines) + 1))


@pytest.mark.parametrize("name", ["A1", "A4", "C1", "C2", "D1", "D2", "E1", "E3"])  # (E4 trains under another threshold than it loads with: the C++ API only)
def test_cli_computes_the_skipgrams_of_a_loaded_model(tmp_path, name):
    import oracle
    from test_host_face import parse_model
    c, _, want, err = mm.fixture(name)
    assert c["load"]["t"] == c["t"] and c["load"]["l"] == c["l"]
    model = model_file(c["model"], tmp_path)
    _, tokens, types, _, _ = parse_model(model)
    data = os.path.join(GOLDEN, c["corpus"] + ".colibri.dat")
    want_bytes = {b"".join(k): refs for k, refs in want.items()}
    for with_corpus in (True, False):
        out = str(tmp_path / ("out%d.colibri.patternmodel" % with_corpus))
        p = subprocess.run([CLI, "-i", model] + (["-f", data] if with_corpus else []) + ["-s"] + cli_options(c) + ["-o", out], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
        assert in_order(["Computing skipgrams"] + err, p.stderr), p.stderr  # the reference's lines, D1's wrapped `total kept` included
        mtype, got_tokens, got_types, counts, refs = parse_model(out)
        assert (mtype, got_tokens, got_types) == (20, tokens, types)
        assert refs == want_bytes and counts == {k: len(v) for k, v in want_bytes.items()}
    if oracle.have_ref():  # the real reference reads the file this build wrote
        dump = str(tmp_path / "d.txt")
        subprocess.check_call([oracle.REF_DRIVER, "load", out, "i", dump])
        got = oracle.parse_dump(open(dump).read(), indexed=True)
        assert (got.tokens, got.types) == (tokens, types) and {k: sorted(v) for k, v in got.refs.items()} == want_bytes


def test_cli_leaves_a_model_that_holds_skipgrams_as_it_is(tmp_path):
    data, cls = os.path.join(GOLDEN, "hamlet.v2.colibri.dat"), os.path.join(GOLDEN, "hamlet.colibri.cls")
    model = str(tmp_path / "is.colibri.patternmodel")
    p = subprocess.run([CLI, "-f", data, "-s", "-t", "2", "-l", "5", "-o", model], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    plain = subprocess.run([CLI, "-i", model, "-c", cls, "-P"], capture_output=True, text=True)
    again = subprocess.run([CLI, "-i", model, "-c", cls, "-s", "-P"], capture_output=True, text=True)
    assert plain.returncode == 0 and again.returncode == 0, plain.stderr + again.stderr
    assert again.stdout == plain.stdout and len(plain.stdout.splitlines()) == 117
    assert "holds skipgrams already: they are not computed again" in again.stderr and "Computing skipgrams" not in again.stderr
    assert "not computed again" not in plain.stderr


def test_cli_refusals(tmp_path):
    model = os.path.join(mm.FIXTURES, "hamlet.v2.i.t2l5.patternmodel")
    data = os.path.join(GOLDEN, "hamlet.v2.colibri.dat")
    p = subprocess.run([CLI, "-i", model, "-s", "--gpus", "2", "-o", str(tmp_path / "o")], capture_output=True, text=True)
    assert p.returncode == 2 and "--gpus" in p.stderr and not os.path.exists(tmp_path / "o")
    p = subprocess.run([CLI, "-i", model, "-f", data, "-e", "100", "-s"], capture_output=True, text=True)  # (as before)
    assert p.returncode == 2 and "can not be combined with -s" in p.stderr
    p = subprocess.run([CLI, "-i", model, "-f", data, "-F", "S"], capture_output=True, text=True)  # (as before)
    assert p.returncode == 2 and "-F S on a loaded model" in p.stderr


# ---- the C++ face: train() without skipgrams, then trainskipgrams(options) in one process ---------------------------------------------------------------
@pytest.mark.parametrize("form", ["flat", "map"])
@pytest.mark.parametrize("corpus,isgold,T", [("hamlet.v2", "hamlet.v2.is.l5.txt", 2), ("zipf20k", "zipf20k.isT1.l5.txt", 1)])
def test_cxx_trainskipgrams_after_train_equals_the_direct_build(tmp_path, corpus, isgold, T, form):
    import oracle
    from test_host_face import parse_model
    want = oracle.parse_dump(open(os.path.join(GOLDEN, isgold)).read(), indexed=True)
    out = str(tmp_path / "m.colibri.patternmodel")
    p = subprocess.run([os.path.join(BIN, "host_selftest"), "trainskipgrams", os.path.join(GOLDEN, corpus + ".colibri.dat"), "5", "2", str(T), form, out], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    mtype, tokens, types, counts, refs = parse_model(out)
    assert (mtype, tokens, types) == (20, want.tokens, want.types)
    assert counts == want.counts and {k: sorted(v) for k, v in refs.items()} == {k: sorted(v) for k, v in want.refs.items()}
    nskip = sum(1 for k in counts if mm.GAP in mm.tokens_of(k))
    assert p.stdout.split() == [str(len(counts)), str(nskip), "1", str(want.tokens), str(want.types)]
    assert "Finding skipgrams on the basis of extracted n-grams..." in p.stderr and "total kept" in p.stderr


def test_cxx_trainskipgrams_on_the_resident_model(tmp_path):
    """a train() that asked for skipgrams at MAXLENGTH 2 leaves the model in HBM and no skipgram: trainskipgrams looks at it there and finds nothing"""
    from test_host_face import parse_model
    out = str(tmp_path / "m.colibri.patternmodel")
    p = subprocess.run([os.path.join(BIN, "host_selftest"), "trainskipgrams", os.path.join(GOLDEN, "hamlet.v2.colibri.dat"), "5", "2", "1", "resident", out], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert in_order(["Counting 3-skipgrams", " None found"], p.stderr)
    _, _, _, counts, _ = parse_model(out)
    assert counts and max(len(mm.tokens_of(k)) for k in counts) == 2 and p.stdout.split()[:2] == [str(len(counts)), "0"]
