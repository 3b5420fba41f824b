"""The three relations of skipgrams on the device (colibri_relations with COLIBRI_REL_INSTANCES / COLIBRI_REL_TEMPLATES, colibri_skipcontent;
colibri-patternmodeller --skipcontent under COLIBRI_SKIPREL=device), against the reference's per-pattern functions (tests/golden/skiprel/) and
the restatement in test_skiprel.py."""
import os
import subprocess

import pytest

from conftest import GOLDEN
from test_cooc import CLI, key_tokens
from test_gpu_cooc import flat
from test_gpu_relations import check_order, exported, rows_of
from test_oracle import read_payload
from test_skiprel import FUNCTIONS, GAP, MODELS, THRESHOLDS, load_fixture, load_model, selftest_rows, skiprel

pytestmark = pytest.mark.gpu
KINDS = {"getinstances": 4, "gettemplates": 5}
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def ctx():
    from colibri_amd import capi
    with capi.Context(0) as c:
        yield c


def sk_rows(keys, a, pb, c, contents):
    """[((A, content), count)] in output order; pattern_b is the content's own number in the model, or NONE when the model does not hold it"""
    number = {k: j for j, k in enumerate(keys)}
    for b, content in zip(pb.tolist(), contents):
        assert b == number.get(content, NONE), content
    return [((keys[x], y), int(z)) for x, y, z in zip(a.tolist(), contents, c.tolist())]


def device_rows(ctx, model, payload, fn, thr=0):
    """fn over a loaded model (flat(): keys in byte order), the row order checked"""
    keys, key_off, kb, ref_off, rs, rt = model
    ctx.upload(payload)
    if fn == "getskipcontent":
        rows = sk_rows(keys, *ctx.skipcontent(key_off, kb, ref_off, rs, rt))
    else:
        rows = rows_of(keys, *ctx.relations(key_off, kb, ref_off, rs, rt, KINDS[fn], threshold=thr))
    check_order(rows, {k: j for j, k in enumerate(keys)})
    return rows


def resident_rows(ctx, keys, fn, thr=0):
    if fn == "getskipcontent":
        rows = sk_rows(keys, *ctx.skipcontent_resident())
    else:
        rows = rows_of(keys, *ctx.relations_resident(KINDS[fn], threshold=thr))
    check_order(rows, {k: j for j, k in enumerate(keys)})
    return rows


def thresholds(fn):
    return (0,) if fn == "getskipcontent" else THRESHOLDS


@pytest.mark.parametrize("corpus,tag", MODELS)
def test_loaded_model_matches_the_reference(ctx, corpus, tag):
    counts, refs, _, _ = load_model(corpus, tag)
    model, payload = flat(counts, refs), read_payload(corpus)
    for fn in FUNCTIONS:
        for thr in thresholds(fn):
            rows = device_rows(ctx, model, payload, fn, thr)
            want = load_fixture(fn, corpus, tag, thr)
            assert dict(rows) == want and len(rows) == len(want), (fn, thr)
    assert ctx.skipcontent_info()[3:] == (1, 0)  # one identity round, no reference skipped


@pytest.mark.parametrize("corpus,tag", MODELS)
def test_resident_model_matches_the_reference(ctx, corpus, tag):
    """the model trained on the device with the fixtures' options is the reference's dump; its resident calls give the reference's rows"""
    ctx.upload(read_payload(corpus))
    ctx.train(mintokens=2, maxlength=5, indexed=1, doskipgrams=True, minskiptypes=1 if tag == "isT1" else 2)
    keys, cnt, refs = exported(ctx)
    counts, want_refs, _, _ = load_model(corpus, tag)
    assert cnt == counts and refs == want_refs
    for fn in FUNCTIONS:
        for thr in thresholds(fn):
            assert dict(resident_rows(ctx, keys, fn, thr)) == load_fixture(fn, corpus, tag, thr), (fn, thr)


@pytest.mark.parametrize("corpus,tag", [("hamlet.v2", "isT1"), ("phrases15k", "is")])
def test_forced_small_chunks_give_the_same_rows(ctx, corpus, tag, monkeypatch):
    """COLIBRI_REL_CHUNK of 1 / 5 / 7 events: chunks cut inside patterns, the runs of a cut pattern carried and merged before the threshold;
    the rows are those of one chunk, in the same order"""
    counts, refs, _, _ = load_model(corpus, tag)
    model, payload = flat(counts, refs), read_payload(corpus)
    info = {"getskipcontent": lambda: ctx.skipcontent_info()[:3]}
    for fn in FUNCTIONS:
        for thr in thresholds(fn)[-1:]:
            one = device_rows(ctx, model, payload, fn, thr)
            events1, chunks1, _ = info.get(fn, ctx.relations_info)()
            assert chunks1 == 1 and events1 >= sum(c for _, c in one) > 0
            for budget in ("1", "5", "7"):
                monkeypatch.setenv("COLIBRI_REL_CHUNK", budget)
                many = device_rows(ctx, model, payload, fn, thr)
                events, chunks, _ = info.get(fn, ctx.relations_info)()
                monkeypatch.delenv("COLIBRI_REL_CHUNK")
                assert events == events1 and chunks >= events // int(budget)
                assert many == one, (fn, thr, budget)


def test_narrow_hashes_give_the_same_rows(ctx, monkeypatch):
    """COLIBRI_SKC_HASH_BITS of 1 / 3 / 8 on phrases15k.isT1 (4840 distinct contents from 10 544 references): different contents share a hash,
    the byte checks tell them apart and the further rounds number them; the rows do not change"""
    counts, refs, _, _ = load_model("phrases15k", "isT1")
    model, payload = flat(counts, refs), read_payload("phrases15k")
    one = device_rows(ctx, model, payload, "getskipcontent")
    assert len(one) == 4840 and ctx.skipcontent_info()[0] == 10544 and ctx.skipcontent_info()[3] == 1
    for bits in ("8", "3", "1"):
        monkeypatch.setenv("COLIBRI_SKC_HASH_BITS", bits)
        narrow = device_rows(ctx, model, payload, "getskipcontent")
        rounds = ctx.skipcontent_info()[3]
        monkeypatch.delenv("COLIBRI_SKC_HASH_BITS")
        assert rounds > 1 and narrow == one, bits


def test_skipgrams_only(ctx):
    """zipf20k.is without its n-grams: the contents are the same (they are slices of the corpus), none of them is in the model, no instance is,
    and the templates that are left relate skipgrams to skipgrams"""
    counts, refs, _, _ = load_model("zipf20k", "is")
    skips = {k: c for k, c in counts.items() if GAP in key_tokens(k)}
    model, payload = flat(skips, refs), read_payload("zipf20k")
    keys, key_off, kb, ref_off, rs, rt = model
    ctx.upload(payload)
    a, pb, c, contents = ctx.skipcontent(key_off, kb, ref_off, rs, rt)
    assert {(keys[x], y): int(z) for x, y, z in zip(a.tolist(), contents, c.tolist())} == load_fixture("getskipcontent", "zipf20k", "is")
    assert len(pb) == 748 and (pb == NONE).all()
    assert device_rows(ctx, model, payload, "getinstances") == []
    templates = dict(device_rows(ctx, model, payload, "gettemplates"))
    assert templates == {k: v for k, v in load_fixture("gettemplates", "zipf20k", "is").items() if k[0] in skips} and templates


def test_two_hundred_thousand_tokens_against_the_restatement(ctx, monkeypatch):
    """a Zipf corpus with injected phrases, trained resident (seed and options picked on the CPU with oracle.train for the three properties asserted
    below); every pattern, all three kinds, in chunks of 4096 events"""
    from colibri_amd import synth
    payload = synth.zipf_corpus(200_000, 500, 7, phrases=True, header=False)
    ctx.upload(payload)
    ctx.train(mintokens=5, maxlength=4, indexed=1, doskipgrams=True, minskiptypes=2)
    keys, cnt, refs = exported(ctx)
    want = skiprel("getskipcontent", cnt, refs, payload)
    assert sum(len(refs[k]) for k in keys if GAP in key_tokens(k)) >= 10 ** 4
    assert max(len(key_tokens(b)) for _, b in want) >= 2 and max(want.values()) >= 100
    monkeypatch.setenv("COLIBRI_REL_CHUNK", "4096")
    assert dict(resident_rows(ctx, keys, "getskipcontent")) == want
    events, chunks, _, rounds, skipped = ctx.skipcontent_info()
    assert events == sum(want.values()) and chunks >= 2 and (rounds, skipped) == (1, 0)
    for fn in ("getinstances", "gettemplates"):
        for thr in (0, 5):
            assert dict(resident_rows(ctx, keys, fn, thr)) == skiprel(fn, cnt, refs, payload, thr), (fn, thr)
            assert ctx.relations_info()[1] >= 2 or thr


def test_refusals(ctx):
    from colibri_amd import capi
    counts, refs, _, _ = load_model("hamlet.v2", "is")
    keys, key_off, kb, ref_off, rs, rt = flat(counts, refs)
    ctx.upload(read_payload("hamlet.v2"))
    with pytest.raises(capi.ColibriError) as e:
        ctx.relations(key_off, kb, ref_off, rs, rt, 6)
    assert e.value.code == capi.ERR_ARG
    flex = dict(counts)
    flex[b"\x06\x04\x07"] = 1
    frefs = dict(refs)
    frefs[b"\x06\x04\x07"] = [(1, 0)]
    fkeys, fko, fkb, fro, frs, frt = flat(flex, frefs)
    for call in (lambda: ctx.relations(fko, fkb, fro, frs, frt, 4), lambda: ctx.relations(fko, fkb, fro, frs, frt, 5), lambda: ctx.skipcontent(fko, fkb, fro, frs, frt)):
        with pytest.raises(capi.ColibriError) as e:
            call()
        assert e.value.code == capi.ERR_UNSUPPORTED
    ctx.train(mintokens=2, maxlength=3, indexed=0)  # an unindexed resident model
    for call in (lambda: ctx.relations_resident(4), lambda: ctx.relations_resident(5), ctx.skipcontent_resident):
        with pytest.raises(capi.ColibriError) as e:
            call()
        assert e.value.code == capi.ERR_STATE
    with capi.Context(0) as bare:  # no corpus
        for call in (lambda: bare.relations(key_off, kb, ref_off, rs, rt, 4), lambda: bare.skipcontent(key_off, kb, ref_off, rs, rt), bare.skipcontent_resident):
            with pytest.raises(capi.ColibriError) as e:
                call()
            assert e.value.code == capi.ERR_STATE


@pytest.mark.parametrize("fn", FUNCTIONS)
def test_cxx_face_device_rows(tmp_path, fn):
    """computerelations_device / computeskipcontent_device of a loaded model (host_selftest skiprel_device) give the reference's rows"""
    for thr in thresholds(fn):
        assert selftest_rows(tmp_path, "skiprel_device", "zipf20k", "is", fn, thr) == load_fixture(fn, "zipf20k", "is", thr), thr


def test_cli_skipcontent_from_the_device():
    """--skipcontent under COLIBRI_SKIPREL=device: the reference's lines, within a pattern by count descending; without the variable (or with
    `host` / `auto`) the host loop prints as before"""
    data = os.path.join(GOLDEN, "hamlet.v2.colibri.dat")
    base = [CLI, "-f", data, "-c", os.path.join(GOLDEN, "hamlet.colibri.cls"), "-s", "-T", "1", "-t", "2", "-l", "5", "--skipcontent"]
    env = {k: v for k, v in os.environ.items() if k != "COLIBRI_SKIPREL"}
    out = subprocess.run(base, capture_output=True, text=True, env=dict(env, COLIBRI_SKIPREL="device"))
    assert out.returncode == 0, out.stderr
    want = open(os.path.join(GOLDEN, "relations.hamlet.v2.isT1.skipcontent.txt")).read().splitlines()
    lines = out.stdout.splitlines()
    assert sorted(lines) == want
    block = []
    for ln in lines + [""]:
        if ln.startswith("\t"):
            block.append(int(ln.split("\t")[4]))
        else:
            assert block == sorted(block, reverse=True)
            block = []
    host = subprocess.run(base, capture_output=True, text=True, env=env)
    assert host.returncode == 0 and sorted(host.stdout.splitlines()) == want
    for where in ("host", "auto"):
        again = subprocess.run(base, capture_output=True, text=True, env=dict(env, COLIBRI_SKIPREL=where))
        assert again.returncode == 0 and again.stdout == host.stdout


def test_references_whose_window_leaves_the_sentence_are_skipped(ctx):
    """a loaded model may hold references that run past their sentence, or name a sentence the corpus does not have: all three kinds skip them
    (the hand-worked model of test_skiprel.py, plus a reference into sentence 9 of a corpus of three), and the skip content counts them"""
    A, B, C = b"\x06", b"\x07", b"\x08"
    S = A + GAP + C
    counts = {S: 4, A + B + C: 1}
    payload = A + B + C + b"\x00" + A + B + b"\x00" + C + b"\x00"
    refs = {S: [(1, 0), (2, 0), (2, 1), (9, 0)], A + B + C: [(1, 0)]}
    model = flat(counts, refs)
    assert dict(device_rows(ctx, model, payload, "getskipcontent")) == skiprel("getskipcontent", counts, refs, payload) == {(S, B): 1}
    events, _, _, rounds, skipped = ctx.skipcontent_info()
    assert (events, rounds, skipped) == (1, 1, 3)
    assert dict(device_rows(ctx, model, payload, "getinstances")) == skiprel("getinstances", counts, refs, payload) == {(S, A + B + C): 1}
    assert dict(device_rows(ctx, model, payload, "gettemplates")) == skiprel("gettemplates", counts, refs, payload) == {(A + B + C, S): 1}
