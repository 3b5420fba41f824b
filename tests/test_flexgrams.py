"""Flexgrams abstracted from skipgrams: IndexedPatternModel::computeflexgrams_fromskipgrams
(reference include/patternmodel.h:3724-3744).

CPU: the restatement in oracle/oracle.py against the reference's known answer (src/test.cpp:1441-1443: 22 flexgrams, model size
155) and against dumps of the reference itself (tests/golden/flex.*.txt, written by make_golden.py where the reference's
insert-while-iterating loop stayed stable). GPU: colibri_flexgrams / colibri_flexgrams_fetch through the C ABI against the
restatement — identical flexgram set, counts and reference lists.

tests/flex_models.py holds a second, vectorised restatement (restate: the six arrays colibri_flexgrams_fetch writes, in its order) and
a generator of models with a known group structure; both are pinned here, on the CPU, to the restatement above. The device is held to
restate() array for array, at the sizes where its scans, sorts and grid-stride loops change path, in tests/test_gpu_flexgrams.py.
"""
import glob
import os

import numpy as np
import pytest

from conftest import small_corpora

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _flex_only(model):
    import oracle
    return {k: v for k, v in model.refs.items() if oracle.key_category(k) == 3}


def test_known_answer_hamlet_22_flexgrams():
    """src/test.cpp:1441-1443: the indexed skipgram model of hamlet (133 patterns) yields 22 flexgrams, 155 patterns in all."""
    import oracle
    m = oracle.parse_dump(open(os.path.join(GOLD, "hamlet.v2.is.l100.txt")).read(), indexed=True)
    assert len(m) == 133
    f, found = oracle.flexgrams_from_skipgrams(m)
    assert found == 22 and len(f) == 155


def test_toflexgram_and_category():
    import oracle
    assert oracle.toflexgram(bytes([6, 3, 3, 7, 3, 8])) == bytes([6, 4, 7, 4, 8])  # "To {*} {*} or {*} to" -> "To {**} or {**} to" (test.py:147-151)
    assert oracle.toflexgram(bytes([0x83, 0x03, 3, 9])) == bytes([0x83, 0x03, 4, 9])  # 03 as the low byte of a 2-byte token is no gap
    assert oracle.key_category(bytes([6, 7])) == 1 and oracle.key_category(bytes([6, 3, 7])) == 2 and oracle.key_category(bytes([6, 4, 7])) == 3
    assert oracle.key_category(bytes([6, 3, 7, 4, 8])) == 3


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLD, "flex.*.txt"))), ids=os.path.basename)
def test_restatement_matches_reference_dumps(path):
    """flex.<corpus>.<mode>.txt = the reference's model after computeflexgrams_fromskipgrams; <corpus>.<mode>.l5.txt = before."""
    import oracle
    name = os.path.basename(path)[len("flex."):-len(".txt")]
    before = oracle.parse_dump(open(os.path.join(GOLD, name + ".l5.txt")).read(), indexed=True)
    after = oracle.parse_dump(open(path).read(), indexed=True)
    mine, found = oracle.flexgrams_from_skipgrams(before)
    assert mine.counts == after.counts and mine.refs == after.refs
    assert found == len(after) - len(before) > 0


# ------------------------------------------------------------------------------------------------------------------------------
def _arrays_of(model):
    keys = list(model.refs)
    key_off = np.zeros(len(keys) + 1, dtype=np.uint64)
    key_off[1:] = np.cumsum([len(k) for k in keys])
    ref_off = np.zeros(len(keys) + 1, dtype=np.uint64)
    ref_off[1:] = np.cumsum([len(model.refs[k]) for k in keys])
    kb = np.frombuffer(b"".join(keys) or b"\0", dtype=np.uint8)
    rs = np.array([r[0] for k in keys for r in model.refs[k]], dtype=np.uint32)
    rt = np.array([r[1] for k in keys for r in model.refs[k]], dtype=np.uint16)
    return key_off, kb, ref_off, rs, rt


def _device_flexgrams(ctx, model):
    fo, fk, fc, (fro, frs, frt) = ctx.flexgrams(*_arrays_of(model))
    kb, off, ro = fk.tobytes(), fo.tolist(), fro.tolist()
    rs, rt = frs.tolist(), frt.tolist()
    out = {}
    for j, c in enumerate(fc.tolist()):
        k = kb[off[j]: off[j + 1]]
        assert k not in out
        out[k] = list(zip(rs[ro[j]: ro[j + 1]], rt[ro[j]: ro[j + 1]]))
        assert c == len(out[k])
    return out


@pytest.fixture(scope="module")
def ctx():
    from colibri_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["hamlet.v2.is.l100", "hamlet.v2.is.l5", "hamlet.v2.isT1.l5", "phrases15k.is.l5", "phrases15k.isT1.l5", "zipf20k.is.l5"])
def test_device_flexgrams_on_reference_models(ctx, name):
    import oracle
    m = oracle.parse_dump(open(os.path.join(GOLD, name + ".txt")).read(), indexed=True)
    want, found = oracle.flexgrams_from_skipgrams(m)
    got = _device_flexgrams(ctx, m)
    assert got == _flex_only(want) and len(got) == found


@pytest.mark.gpu
@pytest.mark.parametrize("corpus", ["rand1", "rand2", "zipf20k", "zipf200k_phrases"])
@pytest.mark.parametrize("maxlength,minskiptypes", [(5, 1), (7, 2)])
def test_device_flexgrams_after_device_training(ctx, corpus, maxlength, minskiptypes):
    """train on the device (indexed + skipgrams), export, abstract on the device; the oracle does both steps on the CPU"""
    import oracle
    payload = small_corpora()[corpus]
    ctx.upload(payload)
    ctx.train(mintokens=2, maxlength=maxlength, indexed=1, doskipgrams=1, minskiptypes=minskiptypes)
    key_off, key_bytes, counts, (ref_off, rs, rt) = ctx.export_arrays()
    fo, fk, fc, (fro, frs, frt) = ctx.flexgrams(key_off, key_bytes, ref_off, rs, rt)
    om = oracle.train(payload, 2, maxlength, indexed=True, doskipgrams=True, minskiptypes=minskiptypes)
    want, found = oracle.flexgrams_from_skipgrams(om)
    kb, off, ro = fk.tobytes(), fo.tolist(), fro.tolist()
    got = {kb[off[j]: off[j + 1]]: list(zip(frs[ro[j]: ro[j + 1]].tolist(), frt[ro[j]: ro[j + 1]].tolist())) for j in range(len(fc))}
    assert got == _flex_only(want) and len(got) == found
    assert fc.tolist() == [len(got[kb[off[j]: off[j + 1]]]) for j in range(len(fc))]
    # the same without the host round trip: on the model still resident in HBM
    ro, rk, rc, (rro, rrs, rrt) = ctx.flexgrams_resident()
    assert (ro.tolist(), rk.tobytes(), rc.tolist(), rro.tolist(), rrs.tolist(), rrt.tolist()) == (fo.tolist(), fk.tobytes(), fc.tolist(), fro.tolist(), frs.tolist(), frt.tolist())


@pytest.mark.gpu
def test_resident_flexgrams_need_an_indexed_model(ctx):
    from colibri_amd import capi
    ctx.upload(small_corpora()["rand1"])
    ctx.train(mintokens=2, maxlength=5)
    with pytest.raises(capi.ColibriError):
        ctx.flexgrams_resident()
    ctx.train(mintokens=2, maxlength=5, indexed=1)  # indexed, no skipgrams: nothing to abstract
    fo, fk, fc, _ = ctx.flexgrams_resident()
    assert fc.size == 0 and fo.tolist() == [0]


def _edge_model():
    import oracle
    refs = {
        bytes([6, 3, 7]): [(3, 1), (1, 0)],                    # unsorted on purpose
        bytes([6, 3, 3, 7]): [(1, 0), (2, 5)],                  # same flexgram, one duplicate reference
        bytes([6, 3, 7, 4, 8]): [(9, 9)],                       # has a {**}: category flexgram, ignored
        bytes([0x83, 0x03, 3, 9]): [(70000, 65535)],            # 2-byte token whose low byte is 03
        bytes([6, 3, 7, 3, 3, 3, 8]): [(5, 5)],
        bytes([6, 7, 8]): [(1, 0), (4, 4)],
        bytes([9, 3, 9]): [],                                   # a skipgram without references still names its flexgram
    }
    return oracle.Model(0, 0, {k: len(v) for k, v in refs.items()}, refs)


@pytest.mark.gpu
def test_device_flexgrams_edge_inputs(ctx):
    import oracle
    # no patterns at all / no skipgrams / a pattern that is already a flexgram is not a skipgram / duplicates are kept / unsorted input
    empty = oracle.Model(0, 0, {}, {})
    assert _device_flexgrams(ctx, empty) == {}
    plain = oracle.Model(0, 0, {bytes([6]): 1, bytes([6, 7]): 1}, {bytes([6]): [(1, 0)], bytes([6, 7]): [(1, 0)]})
    assert _device_flexgrams(ctx, plain) == {}
    m = _edge_model()
    want, found = oracle.flexgrams_from_skipgrams(m)
    got = _device_flexgrams(ctx, m)
    assert got == {k: v for k, v in _flex_only(want).items() if k != bytes([6, 3, 7, 4, 8])}
    assert got[bytes([6, 4, 7])] == [(1, 0), (1, 0), (2, 5), (3, 1)]
    assert got[bytes([9, 4, 9])] == []


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["hamlet.v2.is.l5", "edge"])
def test_flexgram_hash_collisions_are_retried_and_after_four_refused(ctx, monkeypatch, name):
    """COLIBRI_FLEX_HASH_BITS=1[:attempts]: with one bit of hash two of any three flexgrams collide, so flex_core's retry loop runs"""
    import oracle
    from colibri_amd import capi
    if name == "edge":
        m = _edge_model()
        mine = {bytes([6, 3, 7, 4, 8])}  # the model's own flexgram is no skipgram: not part of the answer
    else:
        m = oracle.parse_dump(open(os.path.join(GOLD, name + ".txt")).read(), indexed=True)
        mine = set()
    want = {k: v for k, v in _flex_only(oracle.flexgrams_from_skipgrams(m)[0]).items() if k not in mine}
    assert len(want) >= 3
    # a profiled run of the trainer switches the context's kernel events on: every attempt is then one more launch of COLIBRI_K_SKIPGRAM
    ctx.upload(small_corpora()["rand1"])
    ctx.train(mintokens=2, maxlength=2, profile=1)
    # (the library adds a call's events to these counts only when the call succeeds; those of a refused call wait for the next success.
    # So the counts are read round successful calls only, and the training run above takes in whatever an earlier case left waiting.)
    launches = lambda: ctx.kernel_time(capi.K_SKIPGRAM)[1]
    before = launches()
    assert _device_flexgrams(ctx, m) == want
    unhooked = launches() - before
    for attempts in (1, 2, 3):
        monkeypatch.setenv("COLIBRI_FLEX_HASH_BITS", f"1:{attempts}")
        before = launches()
        assert _device_flexgrams(ctx, m) == want, attempts
        assert launches() - before == unhooked + attempts, "every masked attempt collides and is retried; the first unmasked one succeeds"
    for setting in ("1", "1:4"):
        monkeypatch.setenv("COLIBRI_FLEX_HASH_BITS", setting)
        with pytest.raises(capi.ColibriError) as e:
            _device_flexgrams(ctx, m)
        assert "four seeds" in str(e.value)
        with pytest.raises(capi.ColibriError) as e:  # and nothing of an earlier call is left to fetch
            ctx._flexgrams_fetch(len(want), 1, 1)
        assert e.value.code == capi.ERR_STATE
    monkeypatch.delenv("COLIBRI_FLEX_HASH_BITS")
    assert _device_flexgrams(ctx, m) == want


# ---- tests/flex_models.py (the restatement and the generator the device tests of tests/test_gpu_flexgrams.py stand on) pinned to the oracle ----
def _model_of(arrays):
    """oracle.Model of a model in export layout (flex_models.Model)"""
    import oracle
    key_off, key_bytes, ref_off, rs, rt = arrays
    kb, ko, ro, rs, rt = key_bytes.tobytes(), key_off.tolist(), ref_off.tolist(), rs.tolist(), rt.tolist()
    refs = {kb[ko[p]: ko[p + 1]]: list(zip(rs[ro[p]: ro[p + 1]], rt[ro[p]: ro[p + 1]])) for p in range(len(ko) - 1)}
    assert len(refs) == len(ko) - 1, "a model holds every key once"
    return oracle.Model(0, 0, {k: len(v) for k, v in refs.items()}, refs)


def _restated(arrays):
    """flex_models.restate as ([flexgram keys in its order], {key: [(sentence, token)]}); its offsets and counts must agree with each other"""
    import flex_models
    fo, fk, fc, fro, frs, frt = flex_models.restate(*arrays)
    assert (fo.dtype, fk.dtype, fc.dtype, fro.dtype, frs.dtype, frt.dtype) == (np.uint64, np.uint8, np.uint32, np.uint64, np.uint32, np.uint16)
    assert fo.size == fro.size == fc.size + 1 and fo[0] == fro[0] == 0 and fo[-1] == fk.size and fro[-1] == frs.size == frt.size
    assert np.array_equal(np.diff(fro.astype(np.int64)), fc)
    kb, off, ro, rs, rt = fk.tobytes(), fo.tolist(), fro.tolist(), frs.tolist(), frt.tolist()
    keys = [kb[off[j]: off[j + 1]] for j in range(fc.size)]
    assert len(set(keys)) == len(keys)
    return keys, {k: list(zip(rs[ro[j]: ro[j + 1]], rt[ro[j]: ro[j + 1]])) for j, k in enumerate(keys)}


def _check_restate_against_oracle(m):
    """flexgram set, counts, lists and the oracle's `found`; returns restate's keys in its order"""
    import collections
    import oracle
    want, found = oracle.flexgrams_from_skipgrams(m)
    keys, got = _restated(_arrays_of(m))
    assert set(got) == {oracle.toflexgram(k) for k in m.refs if oracle.key_category(k) == 2}
    old = {k for k in m.refs if oracle.key_category(k) == 3}  # flexgrams the model held before: the oracle merges their references in
    assert set(got) - old == set(_flex_only(want)) - old
    assert found == len(got) - len(set(got) & old)
    for k, lst in got.items():
        theirs = sorted(want.refs[k])
        if k in old:  # only what comes from skipgrams is the answer
            theirs = sorted((collections.Counter(theirs) - collections.Counter(m.refs[k])).elements())
            assert len(theirs) == want.counts[k] - m.counts[k]
        assert lst == theirs, k
        assert k in old or len(lst) == want.counts[k]
    lowest = {}
    for p, k in enumerate(m.refs):
        if oracle.key_category(k) == 2:
            lowest.setdefault(oracle.toflexgram(k), p)
    assert keys == sorted(lowest, key=lowest.get), "groups in ascending order of their lowest member"
    return keys


@pytest.mark.parametrize("name", sorted(os.path.basename(p)[:-len(".txt")] for p in glob.glob(os.path.join(GOLD, "*.is*.l5.txt"))) + ["hamlet.v2.is.l100", "edge"])
def test_restate_matches_the_oracle_on_reference_models(name):
    import oracle
    m = _edge_model() if name == "edge" else oracle.parse_dump(open(os.path.join(GOLD, name + ".txt")).read(), indexed=True)
    assert _check_restate_against_oracle(m)


@pytest.mark.parametrize("seed", range(20))
def test_restate_matches_the_oracle_on_generated_models(seed):
    """every family of the generator, shuffled; the group order and the group sizes are also taken from the generator's own structure"""
    import flex_models
    rng = np.random.default_rng(7000 + seed)
    top = [1000, 255, 70000, (1 << 32) - 1][seed % 4]
    arrays, groups = flex_models.family_model(rng, [60, 300, 900, 1900][seed % 4] + seed, sentences=(0 if seed % 3 == 0 else 1, top))
    assert len(arrays.key_off) - 1 <= 2000
    keys = _check_restate_against_oracle(_model_of(arrays))
    assert keys == [g for g, _ in groups]
    assert [m[0] for _, m in groups] == sorted(m[0] for _, m in groups)
    fo, fk, fc, fro, frs, frt = flex_models.restate(*arrays)
    nref = np.diff(arrays.ref_off.astype(np.int64))
    assert fc.tolist() == [int(nref[m].sum()) for _, m in groups]
    assert any(len(m) > 1 for _, m in groups) and any(c == 0 for c in fc.tolist())
    pairs = frs.astype(np.uint64) << np.uint64(16) | frt
    assert any(np.any(np.diff(pairs[int(a): int(b)]) == 0) for a, b in zip(fro[:-1], fro[1:])), "duplicates are planted and kept"


def test_restate_group_order_follows_the_lowest_member():
    """hand-placed: the group whose lowest member is pattern 0 comes first although its other members come last, and so on"""
    import flex_models
    A, B, C = flex_models.fanin(6, 7, 3), flex_models.fanin(8, 9, 2), flex_models.singleton(10, 11)
    pats = [A[2], (flex_models.encode([6, 7]), None), C[0], B[1], B[0], A[0], A[1]]
    arrays, groups = flex_models.build(np.random.default_rng(1), pats, [1] * 7, shuffle=False, plant=False)
    assert groups == [(flex_models.encode([6, 4, 7]), [0, 5, 6]), (flex_models.encode([10, 4, 11]), [2]), (flex_models.encode([8, 4, 9]), [3, 4])]
    keys, got = _restated(arrays)
    assert keys == [g for g, _ in groups] and [len(got[k]) for k in keys] == [3, 1, 2]
    assert _check_restate_against_oracle(_model_of(arrays)) == keys


def test_restate_collapses_every_vocabulary_class_bytewise():
    """every class of the generator's vocabulary (the varint edges, classes with 03 / 04 / 83 / 84 among their bytes) in every position of a
    three-token key, beside a gap, a {**}, a plain word and a gap lookalike: category and collapsed bytes as oracle.key_category / toflexgram say"""
    import itertools
    import flex_models
    import oracle
    assert {127, 128, 16383, 16384, (1 << 21) - 1, 1 << 21, (1 << 28) - 1, 1 << 28, (1 << 32) - 1, 3 + 3 * 128, 4 + 5 * 128, 3 + (3 << 7) + (3 << 14)} <= set(flex_models.VOCAB)
    assert flex_models.varint(3 + 3 * 128) == bytes([0x83, 0x03]) and flex_models.varint(5 + 4 * 128) == bytes([0x85, 0x04])
    assert flex_models.varint(3 + (3 << 7) + (3 << 14)) == bytes([0x83, 0x83, 0x03]) and all(flex_models.varint(c) == oracle.varint(c) for c in flex_models.VOCAB)
    keys = {}
    for c in flex_models.VOCAB:
        for pos in range(3):
            for others in itertools.product([flex_models.SKIP, flex_models.FLEX, 6, 3 + 3 * 128], repeat=2):
                toks = list(others)
                toks.insert(pos, c)
                key, group = flex_models.pattern(toks)
                assert (group is not None) == (oracle.key_category(key) == 2) and (group is None or group == oracle.toflexgram(key)), toks
                assert flex_models.tokens_of(key) == oracle.key_tokens(key) == [flex_models.varint(t) for t in toks]
                keys.setdefault(key, None)
    keys = list(keys)
    n = len(keys)
    arrays = flex_models.assemble(keys, [1] * n, np.arange(1, n + 1), np.zeros(n))  # pattern p holds the one reference (p + 1, 0)
    want = {}
    for p, k in enumerate(keys):
        if oracle.key_category(k) == 2:
            want.setdefault(oracle.toflexgram(k), []).append((p + 1, 0))
    order, got = _restated(arrays)
    assert got == want and order == list(want) and len(want) > 100
    assert all(b"\x03" not in oracle.key_tokens(k) for k in order)
