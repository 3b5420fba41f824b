"""The subsumption prunes on the device (colibri_subsume / colibri_subsume_resident / colibri_subsume_fetch / colibri_subsume_info; the C++ face's
train() and colibri-patternmodeller -p / --prune / --prunesubsumed under COLIBRI_SUBSUME=device), against the restatement of test_subsume.py:
the flags and both count arrays exactly."""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN
from test_cooc import COOC, MODELS
from test_gpu_coverage import varint
from test_host_face import CLI, SELFTEST, parse_model
from test_oracle import read_payload
from test_subsume import RUNS, subsume

pytestmark = pytest.mark.gpu

PS = [(4, 0), (0, 3), (5, 5), (100, 0), (0, 100), (2, 0), (0, 2), (3, 2)]


@pytest.fixture(scope="module")
def ctx():
    from colibri_amd import capi
    with capi.Context(0) as c:
        yield c


def key_arrays(keys):
    key_off = np.cumsum([0] + [len(k) for k in keys]).astype(np.uint64)
    key_bytes = np.frombuffer(b"".join(keys) + b"\0", dtype=np.uint8)[:-1]
    return key_off, key_bytes


def check(ctx, keys, p, S, maxlength=100, resident=False):
    """one call against the restatement: the flags, the counts of both passes by the tokens of the pruned patterns, what the info reports"""
    from colibri_amd import capi
    info = {}
    alive, log = subsume(keys, p, S, maxlength, info)
    if resident:
        keep, non, sub = ctx.subsume(prunenonsubsumed=p, prunesubsumed=S, maxlength=maxlength, resident=True)
    else:
        keep, non, sub = ctx.subsume(*key_arrays(keys), prunenonsubsumed=p, prunesubsumed=S, maxlength=maxlength)
    want = [[0] * capi.MAX_ORDER, [0] * capi.MAX_ORDER]
    for pas, tokens, pruned in log:
        want[pas - 1][tokens] += pruned
    assert keep.tolist() == [1 if k in alive else 0 for k in keys]
    assert non.tolist() == want[0] and sub.tolist() == want[1]
    assert ctx.subsume_kept == len(alive)
    levels, probes, scratch = ctx.subsume_info()
    assert (levels, probes) == (info["levels"], 2 * info["markers"])
    assert scratch > 0 or not keys
    return keep, alive, log


# ---- the fixture models, uploaded ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("corpus,kind", MODELS)
def test_uploaded_model_equals_the_restatement(ctx, corpus, kind):
    keys = list(parse_model(os.path.join(COOC, f"{corpus}.{kind}.colibri.patternmodel"))[3])
    pruned_any = False
    for p, S in PS:
        for maxlength in (100, 3):  # (min(p, MAXLENGTH): the clamp changes the answer at 3)
            _, alive, _ = check(ctx, keys, p, S, maxlength)
            pruned_any |= len(alive) < len(keys)
    assert pruned_any


# ---- resident models ------------------------------------------------------------------------------------------------------------------------------
KINDS = {"u": {}, "i": dict(indexed=1), "is": dict(indexed=1, doskipgrams=1), "us": dict(doskipgrams_exhaustive=1)}


@pytest.mark.parametrize("corpus", ["hamlet.v2", "zipf20k"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_resident_model_equals_the_restatement_and_the_uploaded_form(ctx, corpus, kind):
    ctx.upload(read_payload(corpus))
    ctx.train(mintokens=2, maxlength=5, **KINDS[kind])
    counts, _ = ctx.export_dict()
    key_off, key_bytes, cnt, refs = ctx.export_arrays()
    kb, off = key_bytes.tobytes(), key_off.tolist()
    keys = [kb[off[j]:off[j + 1]] for j in range(len(off) - 1)]  # export order
    assert set(keys) == set(counts) and len(keys) == len(counts)
    for p, S in ((4, 0), (0, 3), (5, 5)):
        res, _, _ = check(ctx, keys, p, S, 5, resident=True)
        up, _, _ = ctx.subsume(key_off, key_bytes, prunenonsubsumed=p, prunesubsumed=S, maxlength=5)
        assert np.array_equal(res, up)
    # the model is left as it was
    again = ctx.export_arrays()
    assert np.array_equal(again[0], key_off) and np.array_equal(again[1], key_bytes) and np.array_equal(again[2], cnt)


def test_resident_needs_a_trained_model():
    from colibri_amd import capi
    with capi.Context(0) as c:
        with pytest.raises(capi.ColibriError) as e:
            c.subsume(prunenonsubsumed=4, resident=True)
        assert e.value.code == capi.ERR_STATE


# ---- hand-made models at the edges -------------------------------------------------------------------------------------------------------------
T1, T1b, T2, T3, T3b, T4, T4b, T4c = varint(5), varint(6), varint(300), varint(20000), varint(20001), varint(3000000), varint(3000001), varint(3000002)
SKIP = bytes([3])


def tok(i):
    return varint(5 + 50 * i)  # distinct tokens of one and two bytes


def mixed_model(n):
    """n patterns of one to three tokens over neighbouring tokens: some subsumed, some not"""
    keys = []
    for i in range(n):
        r = i % 4
        if r < 2 or i < 3:
            keys.append(tok(i))
        elif r == 2:
            keys.append(tok(i - 2) + tok(i - 1))
        else:
            keys.append(tok(i - 3) + tok(i - 2) + tok(i))
    return keys


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257])
def test_pattern_counts_at_the_wave_and_block_edges(ctx, n):
    for p, S in ((3, 0), (0, 3), (2, 2), (0, 0)):
        check(ctx, mixed_model(n), p, S)
    if n >= 3:  # n - 1 unigrams under one bigram: all but two die in one sweep (the counts cross the waves of a block and the blocks), or two
        keys = [tok(i) for i in range(n - 1)] + [tok(0) + tok(1)]
        _, alive, _ = check(ctx, keys, 2, 0)
        assert len(alive) == 3
        _, alive, _ = check(ctx, keys, 0, 2)
        assert len(alive) == n - 2


def test_unigrams_only_and_marks_that_find_nothing(ctx):
    uni = [tok(i) for i in range(100)]
    for p, S in ((4, 0), (0, 4), (100, 100)):
        keep, _, _ = check(ctx, uni, p, S)
        assert keep.all()
        assert ctx.subsume_info()[:2] == (0, 0)
    # lengths 1 and 3 only: the trigrams' marks find no bigram, and no bigram marks the unigrams
    keys = uni + [tok(i) + tok(i + 1) + tok(i + 2) for i in range(70)]
    for p, S in ((3, 0), (0, 3), (3, 3)):
        keep, _, _ = check(ctx, keys, p, S)
        assert keep.all()
    assert ctx.subsume_info()[:2] == (2, 4 * 70)


def test_a_level_wiped_out_leaves_the_next_one_alone(ctx):
    """pass 1 at level 3 kills every bigram (none is a sub-pattern of a trigram); level 2 then has no marking pattern and must prune nothing:
    without the empty rule every unigram would die"""
    uni = [tok(i) for i in range(80)]
    bigrams = [tok(i) + tok(i + 7) for i in range(70)]
    trigrams = [tok(i) + tok(i + 1) + tok(i + 2) for i in range(66)]
    keys = uni + bigrams + trigrams
    keep, alive, log = check(ctx, keys, 3, 0)
    assert log == [(1, 2, 70), (1, 1, 0)] and alive == set(uni + trigrams)
    assert ctx.subsume_info()[:2] == (1, 2 * 66)
    # with one bigram left the level below does prune
    _, alive, log = check(ctx, keys + [tok(0) + tok(1)], 3, 0)
    assert log == [(1, 2, 70), (1, 1, 78)]
    check(ctx, keys, 3, 3)


def test_token_widths_first_and_last(ctx):
    widths = [T1, T2, T3, T4]
    keys = widths + [T1b, T3b, T4b, T4c]
    keys += [a + b for a in widths for b in widths]
    keys += [a + T1b + b for a in widths for b in widths] + [a + T1b for a in widths] + [T1b + b for b in widths[:2]] + [T3b + T1b, T1b + T4c]
    assert len(set(keys)) == len(keys)
    for p, S in ((2, 0), (3, 0), (0, 2), (0, 3), (3, 3)):
        check(ctx, keys, p, S)


def test_slices_of_7_8_9_16_and_17_bytes(ctx):
    """sub-patterns whose bytes take the look-up's word path, its tail path and both; decoys that differ in the last byte, in the first word, in
    the second word"""
    subs = {7: [T4, T3], 8: [T4, T4b], 9: [T4, T4b, T1], 16: [T4, T4b, T4, T4b], 17: [T4, T4b, T4, T4b, T1]}
    keys = [T1, T2]
    for L, toks in subs.items():
        s = b"".join(toks)
        assert len(s) == L
        last = {T3: T3b, T4b: T4c, T1: T1b}[toks[-1]]
        keys += [s, b"".join(toks[:-1]) + last, T4c + b"".join(toks[1:]), s + T1, T2 + s]
        if len(toks) >= 4:
            keys.append(b"".join(toks[:2]) + T4c + b"".join(toks[3:]))
    keys = list(dict.fromkeys(keys))
    for p, S in ((6, 0), (0, 6), (6, 6), (3, 0), (4, 2)):
        check(ctx, keys, p, S)


def test_skipgrams_and_a_pattern_that_is_its_own_sub_pattern_twice(ctx):
    a, b = T1, T2
    keys = [a, b, SKIP, a + b, a + SKIP, SKIP + b, SKIP + SKIP, b + SKIP, a + SKIP + b, a + SKIP + SKIP, SKIP + SKIP + b, a + SKIP + SKIP + b, b + SKIP + a]
    for p, S in ((4, 0), (0, 4), (4, 4), (3, 0), (2, 0)):
        check(ctx, keys, p, S)
    _, alive, _ = check(ctx, [a + SKIP + b, a + SKIP, SKIP + b, a + b], 3, 0)
    assert alive == {a + SKIP + b, a + SKIP, SKIP + b}
    keys = [a, a + a, a + a + a, b, b + b]
    for p, S in ((3, 0), (0, 3), (3, 3)):
        check(ctx, keys, p, S)


# ---- hash collisions ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [1, 4])
def test_hash_collisions_leave_identity_to_the_bytes(ctx, monkeypatch, bits):
    monkeypatch.setenv("COLIBRI_SUBSUME_HASH_BITS", str(bits))
    keys = list(parse_model(os.path.join(COOC, "zipf20k.is.colibri.patternmodel"))[3])
    for p, S in ((4, 0), (0, 3), (5, 5)):
        check(ctx, keys, p, S)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    from colibri_amd import capi
    with capi.Context(0) as fresh:
        assert fresh.L.colibri_subsume_fetch(fresh.h, None, None, None) == capi.ERR_STATE
    keys = [T1, T2, T1 + T2]
    for p, S in ((-1, 0), (0, -1)):
        with pytest.raises(capi.ColibriError) as e:
            ctx.subsume(*key_arrays(keys), prunenonsubsumed=p, prunesubsumed=S)
        assert e.value.code == capi.ERR_ARG
    with pytest.raises(capi.ColibriError) as e:
        ctx.subsume(*key_arrays(keys + [T1 + bytes([4]) + T2]), prunenonsubsumed=3)
    assert e.value.code == capi.ERR_UNSUPPORTED and "flexgram" in str(e.value)
    assert ctx.L.colibri_subsume_fetch(ctx.h, None, None, None) == capi.ERR_STATE  # (a refused call leaves no result)
    with pytest.raises(capi.ColibriError) as e:  # colibri_train goes on refusing the options, and says whose pass it is
        ctx.upload(read_payload("hamlet.v2"))
        ctx.train(mintokens=2, maxlength=5, prunenonsubsumed=4)
    assert e.value.code == capi.ERR_UNSUPPORTED and "colibri_subsume_resident" in str(e.value)
    check(ctx, keys, 3, 0)  # the context goes on working


# ---- the C++ face and the CLI ---------------------------------------------------------------------------------------------------------------------
COMMANDS = {"selftest p4": "p4", "selftest S3": "S3", "-p 4": "p4", "--prune 4": "p4", "--prunesubsumed 3": "S3", "-p 5 --prunesubsumed 5": "p5S5"}
CLI_KIND = {"u": ["-u"], "i": [], "us": ["-u", "-s"], "is": ["-s"]}


def wanted(corpus, kind, tag):
    """the reference's model after the prunes: its golden, or (u / i at p5S5, which has none) the restatement on its golden unpruned model"""
    import oracle
    indexed = kind in ("i", "is")
    path = os.path.join(GOLDEN, f"subsumption.{corpus}.{kind}.{tag}.txt")
    if os.path.exists(path):
        levels = json.load(open(os.path.join(GOLDEN, "subsumption.levels.json")))[f"{corpus}.{kind}.{tag}"]
        return oracle.parse_dump(open(path).read(), indexed=indexed), [tuple(e) for e in levels]
    before = oracle.parse_dump(open(os.path.join(GOLDEN, f"{corpus}.{kind}.l5.txt")).read(), indexed=indexed)
    alive, log = subsume(list(before.counts), *RUNS[tag], 5)
    return oracle.Model(before.tokens, before.types, {k: before.counts[k] for k in alive}, {k: before.refs[k] for k in alive} if indexed else None), log


def prune_lines(err):
    return [ln for ln in err.splitlines() if ln.startswith(" pruned ") or ln.startswith("Pruning ")]


@pytest.mark.parametrize("corpus", ["hamlet.v2", "zipf20k"])
@pytest.mark.parametrize("kind", list(CLI_KIND))
@pytest.mark.parametrize("command", list(COMMANDS))
def test_cxx_face_and_cli_on_the_device_route(tmp_path, corpus, kind, command):
    tag = COMMANDS[command]
    data = os.path.join(GOLDEN, corpus + ".colibri.dat")
    want, levels = wanted(corpus, kind, tag)
    out = {}
    for route in ("device", "host"):
        model = str(tmp_path / f"{route}.colibri.patternmodel")
        if command.startswith("selftest"):
            args = [SELFTEST, "gpu", data, model, kind, "5", "2", tag]
        else:
            args = [CLI, "-f", data, "-t", "2", "-l", "5", "-o", model] + CLI_KIND[kind] + command.split()
        p = subprocess.run(args, capture_output=True, text=True, env={**os.environ, "COLIBRI_SUBSUME": route}, timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
        out[route] = (open(model, "rb").read(), prune_lines(p.stderr), p.stderr)
        mtype, tokens, types, counts, refs = parse_model(model)
        assert (tokens, types) == (want.tokens, want.types)
        assert counts == want.counts
        if kind in ("i", "is"):
            assert refs == want.refs
    assert out["device"][1] == out["host"][1]
    said = [f" pruned {k} {'non-subsumed' if pas == 1 else 'subsumed'} {t}-grams" for pas, t, k in levels]
    assert [ln for ln in out["device"][1] if ln.startswith(" pruned ")] == said
    assert f"(subsumption prune on the device: {'resident' if kind == 'is' else 'uploaded'} model)" in out["device"][2]
    assert "subsumption prune on the device" not in out["host"][2]
    assert sorted(parse_model(str(tmp_path / "device.colibri.patternmodel"))[3].items()) == sorted(parse_model(str(tmp_path / "host.colibri.patternmodel"))[3].items())


def test_auto_goes_to_the_device_from_the_threshold_on(tmp_path):
    """COLIBRI_SUBSUME unset: the host route below COLIBRI_SUBSUME_MIN patterns (unset: 10^6), the device route from there on, silently; the step's
    line under COLIBRI_HOST_TIMING says which"""
    data = os.path.join(GOLDEN, "hamlet.v2.colibri.dat")
    model = str(tmp_path / "m.colibri.patternmodel")
    args = [CLI, "-f", data, "-t", "2", "-l", "5", "-u", "-p", "4", "-o", model]  # 102 patterns
    env = {k: v for k, v in os.environ.items() if k not in ("COLIBRI_SUBSUME", "COLIBRI_SUBSUME_MIN")}
    env["COLIBRI_HOST_TIMING"] = "1"
    lines = None
    for minimum, route in ((None, "host"), ("102", "device"), ("103", "host")):
        p = subprocess.run(args, capture_output=True, text=True, env=env if minimum is None else {**env, "COLIBRI_SUBSUME_MIN": minimum}, timeout=300)
        assert p.returncode == 0, p.stderr
        assert f"COLIBRI_HOST_TIMING subsume" in p.stderr and f" ms on the {route}, 62 patterns left" in p.stderr
        assert "subsumption prune on the device" not in p.stderr
        assert " pruned 34 non-subsumed 1-grams" in p.stderr
        lines = lines or prune_lines(p.stderr)
        assert prune_lines(p.stderr) == lines
        assert len(parse_model(model)[3]) == 62
