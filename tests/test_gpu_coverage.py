"""The coverage report on the device (colibri_coverage / colibri_coverage_resident; colibri-patternmodeller -R / -r under COLIBRI_REPORT), against the
restatement of test_coverage.py and the reference's text in tests/golden/views/. Every value is an integer: all comparisons are exact."""
import os
import random
import subprocess

import numpy as np
import pytest

from test_coverage import coverage_groups, load_case
from test_views import CASES, CLI, GOLD, VIEWS, golden

pytestmark = pytest.mark.gpu

VALUES = ("patterns", "counts", "types", "tokens")


@pytest.fixture(scope="module")
def ctx():
    from colibri_amd import capi
    with capi.Context(0) as c:
        yield c


def varint(cls):
    out = []
    while cls >= 128:
        out.append((cls & 127) | 128)
        cls >>= 7
    return bytes(out + [cls])


def flat(refs, counts=None):
    """{key: [(sentence, token)]} (and {key: count} for an unindexed model) in export layout, keys in byte order"""
    keys = sorted(refs if refs is not None else counts)
    key_off = np.cumsum([0] + [len(k) for k in keys]).astype(np.uint64)
    kb = np.frombuffer(b"".join(keys), dtype=np.uint8)
    if refs is None:
        return key_off, kb, np.array([counts[k] for k in keys], dtype=np.uint32), None
    ref_off = np.cumsum([0] + [len(refs[k]) for k in keys]).astype(np.uint64)
    rs = np.array([s for k in keys for s, _ in refs[k]], dtype=np.uint32)
    rt = np.array([t for k in keys for _, t in refs[k]], dtype=np.uint16)
    return key_off, kb, None, (ref_off, rs, rt)


def device(ctx, key_off, kb, counts, refs, per_size=False):
    return ctx.coverage(key_off, kb, counts, *(refs if refs is not None else (None, None, None)), per_size=per_size)


def assert_same(got, want, what=""):
    for name, g, w in zip(VALUES, got, want):
        assert g.shape == w.shape and np.array_equal(g, w), (what, name, g.tolist(), w.tolist())


def check(ctx, key_off, kb, counts, refs, what=""):
    for per_size in (False, True):
        assert_same(device(ctx, key_off, kb, counts, refs, per_size), coverage_groups(key_off, kb, counts, refs, per_size), (what, per_size))


def cli(args, **env):
    p = subprocess.run([CLI] + args, capture_output=True, env={**os.environ, **env}, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    return p.stdout, p.stderr.decode()


# ---- the golden view cases ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_loaded_golden_models(ctx, case):
    indexed, tokens, types, key_off, kb, counts, refs = load_case(case)
    check(ctx, key_off, kb, None if indexed else counts, refs, case)
    if indexed:
        assert ctx.coverage_info()[0] == len(refs[1])
    args = ["-i", os.path.join(VIEWS, f"{case}.colibri.patternmodel"), "-c", os.path.join(GOLD, CASES[case][2])] + ([] if indexed else ["-u"])
    for view, flag in (("report", "-R"), ("simplereport", "-r")):
        out, err = cli(args + [flag], COLIBRI_REPORT="device")
        assert out == golden(case, view) and "(statistics on the device: uploaded model)" in err
        assert cli(args + [flag], COLIBRI_REPORT="host")[0] == out


@pytest.mark.parametrize("case", list(CASES))
def test_golden_models_trained_on_the_device(case):
    corpus, flags, cls = CASES[case]
    resident = "-s" in flags and "-u" not in flags  # the trainings that leave their model in HBM: indexed with skipgrams
    args = ["-f", os.path.join(GOLD, f"{corpus}.colibri.dat"), "-c", os.path.join(GOLD, cls)] + flags
    for view, flag in (("report", "-R"), ("simplereport", "-r")):
        out, err = cli(args + [flag], COLIBRI_REPORT="device")
        assert out == golden(case, view)
        assert f"(statistics on the device: {'resident' if resident else 'uploaded'} model)" in err
        assert cli(args + [flag], COLIBRI_REPORT="host")[0] == out


def test_resident_form_through_the_python_face(ctx):
    """the model of a train() on this context, where it lies: the values of the same model exported and uploaded again"""
    from test_oracle import read_payload
    ctx.upload(read_payload("hamlet.v2"))
    ctx.train(mintokens=2, maxlength=5, indexed=1, doskipgrams=True, minskiptypes=2)
    key_off, key_bytes, counts, (ref_off, rs, rt) = ctx.export_arrays()
    kb = key_bytes[: int(key_off[-1])]
    for per_size in (False, True):
        got = ctx.coverage_resident(per_size=per_size)
        assert_same(got, coverage_groups(key_off, kb, None, (ref_off, rs, rt), per_size))
        assert_same(ctx.coverage(key_off, kb, counts, ref_off, rs, rt, per_size=per_size), got)
    from colibri_amd import capi
    ctx.train(mintokens=2, maxlength=3, indexed=0)
    with pytest.raises(capi.ColibriError) as e:
        ctx.coverage_resident()
    assert e.value.code == -6  # COLIBRI_ERR_STATE: not an indexed model


# ---- random indexed models ---------------------------------------------------------------------------------------------------------------------
def random_model(seed, first_sentence, skipgrams):
    """every n-gram (n <= 5) of a few hundred random tokens in sentences of 1..40 tokens that occurs twice, and with `skipgrams` its gapped forms"""
    rnd = random.Random(seed)
    refs = {}
    for s in range(first_sentence, first_sentence + 18):
        sent = [rnd.choice([5, 6, 7, 8, 9, 130, 131, 20000]) for _ in range(rnd.randint(1, 40))]
        for t in range(len(sent)):
            for n in range(1, 6):
                if t + n > len(sent):
                    break
                w = sent[t:t + n]
                refs.setdefault(b"".join(varint(x) for x in w), []).append((s, t))
                if skipgrams and n >= 3:
                    for mask in range(1, 1 << (n - 2)):
                        g = [3 if 0 < i < n - 1 and (mask >> (i - 1)) & 1 else x for i, x in enumerate(w)]
                        refs.setdefault(b"".join(varint(x) for x in g), []).append((s, t))
    return {k: v for k, v in refs.items() if len(v) >= 2}


@pytest.mark.parametrize("skipgrams", [False, True])
@pytest.mark.parametrize("first_sentence", [1, 100000])
def test_random_indexed_models(ctx, first_sentence, skipgrams):
    for seed in (1, 2):
        refs = random_model(seed, first_sentence, skipgrams)
        assert any(len(v) > 20 for v in refs.values()) and (not skipgrams or any(b"\x03" in k for k in refs))
        check(ctx, *flat(refs), what=(seed, first_sentence, skipgrams))


# ---- models written by hand --------------------------------------------------------------------------------------------------------------------
def test_a_pattern_of_forty_tokens_spans_three_bitmap_words(ctx):
    long = b"".join(varint(10 + i) for i in range(40))
    refs = {long: [(1, 0), (1, 30), (2, 27), (7, 65530)], varint(10): [(1, 0), (2, 5), (2, 66)], varint(11) + varint(12): [(2, 0), (9, 3)]}
    key_off, kb, _, flat_refs = flat(refs)
    check(ctx, key_off, kb, None, flat_refs)
    want = coverage_groups(key_off, kb, None, flat_refs, True)
    assert int(want[3][0][40]) == 70 + 40 + 40  # (1, 0..69); (2, 27..66); (7, 65530..65535) and (7, 0..33): token indices wrap at 16 bits


def test_class_ids_at_the_word_edge_and_multi_byte_tokens(ctx):
    ids = [31, 32, 127, 128, 2 ** 14 + 5, 2 ** 21 - 1]
    refs = {varint(c): [(1, j)] for j, c in enumerate(ids)}
    refs[varint(31) + varint(128)] = [(1, 0)]
    refs[varint(32) + varint(3) + varint(2 ** 14 + 5)] = [(1, 1)]
    assert len(varint(2 ** 14 + 5)) == 3
    check(ctx, *flat(refs))
    assert int(device(ctx, *flat(refs))[2][0][0]) == len(ids) + 1  # the gap is a type


def test_an_empty_model(ctx):
    got = ctx.coverage(np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint32))
    assert all(a.shape == (4, 0) for a in got)
    assert ctx.coverage_info() == (0, 0, 0)


def test_an_indexed_model_of_unigrams_only(ctx):
    refs = {varint(c): [(s, t) for s in range(1, 4) for t in range(c % 7)] for c in range(5, 40)}
    refs[varint(7)] = []
    check(ctx, *flat(refs))


def test_an_unindexed_model(ctx):
    counts = {varint(5): 9, varint(5) + varint(6): 4, varint(5) + varint(3) + varint(6): 2, varint(300): 0, varint(5) + varint(4) + varint(6): 3}
    key_off, kb, cnt, _ = flat(None, counts)
    check(ctx, key_off, kb, cnt, None)
    got = device(ctx, key_off, kb, cnt, None)
    assert int(got[1][0][0]) == 18 and not got[3].any() and ctx.coverage_info()[0] == 0


def test_a_model_with_flexgrams(ctx):
    """the reference's model after computeflexgrams_fromskipgrams: flexgrams are counted like any pattern ({**} is one token), without per-size rows"""
    import oracle
    m = oracle.parse_dump(open(os.path.join(GOLD, "flex.hamlet.v2.is.txt")).read(), indexed=True)
    refs = {k: list(v) for k, v in m.refs.items()}
    assert any(b"\x04" in k for k in refs)
    check(ctx, *flat(refs))
    got = device(ctx, *flat(refs))
    assert got[0][3][0] > 0 and not got[0][3][1:].any() and got[2][3][1:].any()


# ---- balance, budget ---------------------------------------------------------------------------------------------------------------------------
def test_one_pattern_with_seventy_thousand_references(ctx, monkeypatch):
    rnd = random.Random(3)
    refs = random_model(4, 1, True)
    refs[varint(5)] = sorted({(rnd.randint(1, 4000), rnd.randint(0, 60)) for _ in range(90000)})[:70000]
    assert len(refs[varint(5)]) == 70000
    arrays = flat(refs)
    want = {ps: coverage_groups(*arrays[:2], None, arrays[3], ps) for ps in (False, True)}
    for slice_ in (None, "1", "5", "7"):
        if slice_:
            monkeypatch.setenv("COLIBRI_COV_SLICE", slice_)
        for ps in (False, True):
            assert_same(device(ctx, *arrays, per_size=ps), want[ps], (slice_, ps))
    monkeypatch.delenv("COLIBRI_COV_SLICE")
    monkeypatch.setenv("COLIBRI_COV_TEST", "0")  # every touched word gets its atomic: the same bitmap
    assert_same(device(ctx, *arrays, per_size=True), want[True], "no test before set")


def test_a_budget_below_need_is_refused_and_the_cli_falls_back(ctx, monkeypatch):
    from colibri_amd import capi
    case = "hamlet.is"
    indexed, tokens, types, key_off, kb, counts, refs = load_case(case)
    monkeypatch.setenv("COLIBRI_COV_BUDGET", "64")
    with pytest.raises(capi.ColibriError) as e:
        device(ctx, key_off, kb, None, refs)
    assert e.value.code == -7 and "COLIBRI_COV_BUDGET" in str(e.value)  # COLIBRI_ERR_OVERFLOW
    monkeypatch.delenv("COLIBRI_COV_BUDGET")
    args = ["-i", os.path.join(VIEWS, f"{case}.colibri.patternmodel"), "-c", os.path.join(GOLD, CASES[case][2]), "-R"]
    out, err = cli(args, COLIBRI_REPORT="auto", COLIBRI_REPORT_MIN="1", COLIBRI_COV_BUDGET="64")
    assert out == golden(case, "report") and "(coverage on the host: " in err
    p = subprocess.run([CLI] + args, capture_output=True, env={**os.environ, "COLIBRI_REPORT": "device", "COLIBRI_COV_BUDGET": "64"}, timeout=300)
    assert p.returncode != 0 and b"COLIBRI_COV_BUDGET" in p.stderr  # device: loud, no fallback
    out, err = cli(args, COLIBRI_REPORT="auto")
    assert out == golden(case, "report") and "on the device" not in err  # a model this small stays on the host
