"""Sentence co-occurrence on the device (colibri_cooc / colibri_cooc_resident; colibri-patternmodeller -C / -Y), against the reference's
per-pattern getcooc (tests/golden/cooc/) and the restatement in test_cooc.py."""
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN
from test_cooc import CLI, COOC, MODELS, THRESHOLDS, cooc, key_tokens, load_fixture, load_model, npmi_rows
from test_oracle import read_payload

pytestmark = pytest.mark.gpu


def flat(counts, refs):
    """a model {key: count}, {key: [(s, t)]} in export layout (keys in byte order)"""
    keys = sorted(counts)
    key_off = np.zeros(len(keys) + 1, dtype=np.uint64)
    key_off[1:] = np.cumsum([len(k) for k in keys])
    ref_off = np.zeros(len(keys) + 1, dtype=np.uint64)
    ref_off[1:] = np.cumsum([len(refs[k]) for k in keys])
    rs = np.array([s for k in keys for s, _ in refs[k]], dtype=np.uint32)
    rt = np.array([t for k in keys for _, t in refs[k]], dtype=np.uint16)
    return keys, key_off, np.frombuffer(b"".join(keys), dtype=np.uint8), ref_off, rs, rt


def rows_of(keys, a, b, c, v):
    return [((keys[x], keys[y]), int(z), float(w)) for x, y, z, w in zip(a.tolist(), b.tolist(), c.tolist(), v.tolist())]


def check_order(rows):
    """values non-increasing; equal values ordered by A's key bytes, then B's"""
    for (k0, _, v0), (k1, _, v1) in zip(rows, rows[1:]):
        assert v0 > v1 or (v0 == v1 and k0 < k1), (k0, v0, k1, v1)


def device_cooc(ctx, counts, refs, payload, thr=0, mode=0, x=0.0):
    keys, key_off, kb, ref_off, rs, rt = flat(counts, refs)
    ctx.upload(payload)
    return keys, rows_of(keys, *ctx.cooc(key_off, kb, ref_off, rs, rt, threshold=thr, mode=mode, npmi_threshold=x))


@pytest.fixture(scope="module")
def ctx():
    from colibri_amd import capi
    with capi.Context(0) as c:
        yield c


@pytest.mark.parametrize("thr", THRESHOLDS)
@pytest.mark.parametrize("corpus,kind", MODELS)
def test_loaded_model_matches_the_references_getcooc(ctx, corpus, kind, thr):
    counts, refs = load_model(corpus, kind)
    _, rows = device_cooc(ctx, counts, refs, read_payload(corpus), thr)
    want = load_fixture(corpus, kind, thr)
    assert {k: c for k, c, _ in rows} == want and len(rows) == len(want)
    check_order(rows)
    assert all(v == c for _, c, v in rows)


@pytest.mark.parametrize("corpus,kind", MODELS)
def test_npmi_matches_the_restatement(ctx, corpus, kind):
    counts, refs = load_model(corpus, kind)
    table = load_fixture(corpus, kind, 0)
    for x in (-1.0, 0.1, 0.5):
        _, rows = device_cooc(ctx, counts, refs, read_payload(corpus), mode=1, x=x)
        want = npmi_rows(counts, table, x)
        got = {k: v for k, _, v in rows}
        near = {k for k, v in want.items() if abs(v - x) < 1e-12}  # (a value at the threshold itself may round either way)
        assert set(got) - near == set(want) - near
        for k in got:
            assert got[k] == pytest.approx(want[k], rel=1e-12, abs=1e-15)
            assert table[k] == next(c for kk, c, _ in rows if kk == k)
        check_order(rows)


@pytest.mark.parametrize("corpus,flags", [("hamlet.v2", dict(doskipgrams=True)), ("edge", dict(doskipgrams=True)), ("zipf20k", {}), ("phrases15k", dict(doskipgrams=True))])
@pytest.mark.parametrize("thr", [0, 2])
def test_resident_model_matches_the_restatement(ctx, corpus, flags, thr):
    payload = read_payload(corpus)
    ctx.upload(payload)
    ctx.train(mintokens=2, maxlength=4, indexed=1, **flags)
    key_off, key_bytes, counts, (ref_off, rs, rt) = ctx.export_arrays()
    kb, off = key_bytes.tobytes(), key_off.tolist()
    keys = [kb[off[j]:off[j + 1]] for j in range(len(counts))]
    cnt = {k: int(c) for k, c in zip(keys, counts.tolist())}
    refs = {k: list(zip(rs[int(ref_off[j]):int(ref_off[j + 1])].tolist(), rt[int(ref_off[j]):int(ref_off[j + 1])].tolist())) for j, k in enumerate(keys)}
    rows = rows_of(keys, *ctx.cooc_resident(threshold=thr))
    assert {k: c for k, c, _ in rows} == cooc(cnt, refs, payload, thr)
    check_order(rows)


@pytest.mark.parametrize("corpus,kind", [("zipf20k", "is"), ("hamlet.v2", "is"), ("phrases15k", "i"), ("edge", "is")])
def test_forced_small_chunks_give_the_same_rows(ctx, corpus, kind, monkeypatch):
    """COLIBRI_COOC_CHUNK below one pattern's events: chunks are cut inside patterns, the runs of a cut pattern are carried and merged before the
    threshold and the NPMI are applied; the rows are those of one chunk, in the same order, and the scratch does not grow"""
    counts, refs = load_model(corpus, kind)
    payload = read_payload(corpus)
    for mode, thr, x in ((0, 2, 0.0), (0, 3, 0.0), (1, 0, 0.2)):
        _, one = device_cooc(ctx, counts, refs, payload, thr, mode, x)
        events1, chunks1, scratch1 = ctx.cooc_info()
        assert chunks1 == 1
        for budget in ("300", "7"):
            monkeypatch.setenv("COLIBRI_COOC_CHUNK", budget)
            _, many = device_cooc(ctx, counts, refs, payload, thr, mode, x)
            events, chunks, scratch = ctx.cooc_info()
            monkeypatch.delenv("COLIBRI_COOC_CHUNK")
            assert events == events1 and chunks >= events // int(budget) > 3
            assert scratch <= scratch1
            assert many == one


def test_a_pattern_spread_over_many_chunks():
    """one pattern with every pair event: a budget of a few events cuts it into hundreds of chunks; its rows are whole"""
    from colibri_amd import capi
    A, B, C = b"\x06", b"\x07", b"\x08"
    payload = (A + C + B + C + A + b"\x00") * 400  # per sentence: A at 0 and 4, B at 2; A-A (gap 3) and A-B, B-A pairs all count
    counts = {A: 800, B: 400}
    refs = {A: [(s, t) for s in range(1, 401) for t in (0, 4)], B: [(s, 2) for s in range(1, 401)]}
    want = {(A, A): 800, (A, B): 800, (B, A): 800}
    with capi.Context(0) as c:
        for budget in (None, "5", "1"):
            if budget:
                os.environ["COLIBRI_COOC_CHUNK"] = budget
            try:
                _, rows = device_cooc(c, counts, refs, payload, 2)
                _, chunks, _ = c.cooc_info()
            finally:
                os.environ.pop("COLIBRI_COOC_CHUNK", None)
            assert {k: n for k, n, _ in rows} == want
            assert chunks >= (1 if budget is None else 2400 // int(budget))


def test_npmi_of_counts_whose_product_passes_2_to_the_32():
    """two patterns of 70 000 references each: c(A) * c(B) = 4.9e9 is a 64-bit product on the device (the reference's counts are size_t)"""
    from colibri_amd import capi
    A, B, C = b"\x06", b"\x07", b"\x08"
    n = 70000
    payload = (A + C + B + b"\x00") * n
    counts = {A: n, B: n}
    refs = {A: [(s, 0) for s in range(1, n + 1)], B: [(s, 2) for s in range(1, n + 1)]}
    with capi.Context(0) as c:
        _, rows = device_cooc(c, counts, refs, payload, mode=1, x=-100.0)
    got = {k: v for k, _, v in rows}
    want = npmi_rows(counts, {(A, B): n, (B, A): n}, -100.0)
    assert set(got) == {(A, B), (B, A)}
    for k in got:
        assert got[k] == pytest.approx(want[k], rel=1e-12)
        wrapped = math.log(n / ((n * n) & 0xFFFFFFFF)) / -math.log(n / (2 * n))
        assert got[k] != pytest.approx(wrapped, rel=1e-6)


def _zipf_model(ctx, ntok, maxlength, seed, thr=2, **flags):
    from colibri_amd import synth
    payload = synth.zipf_corpus(ntok, 2000, seed, header=False)
    ctx.upload(payload)
    ctx.train(mintokens=thr, maxlength=maxlength, indexed=1, **flags)
    key_off, key_bytes, counts, (ref_off, rs, rt) = ctx.export_arrays()
    kb, off = key_bytes.tobytes(), key_off.tolist()
    keys = [kb[off[j]:off[j + 1]] for j in range(len(counts))]
    return payload, keys, counts, ref_off, rs, rt


def test_zipf_corpus_matches_the_restatement(ctx):
    payload, keys, counts, ref_off, rs, rt = _zipf_model(ctx, 300000, 3, 11, thr=40, doskipgrams=True)
    cnt = {k: int(c) for k, c in zip(keys, counts.tolist())}
    refs = {k: list(zip(rs[int(ref_off[j]):int(ref_off[j + 1])].tolist(), rt[int(ref_off[j]):int(ref_off[j + 1])].tolist())) for j, k in enumerate(keys)}
    rows = rows_of(keys, *ctx.cooc_resident(threshold=2))
    assert {k: c for k, c, _ in rows} == cooc(cnt, refs, payload, 2)
    check_order(rows)


def test_ngram_model_events_and_symmetry_at_ten_million_tokens(ctx):
    """threshold 0 on an n-gram model: the joint counts sum to the qualifying occurrence pairs, counted here per sentence from sorted positions,
    and (A, B) has the count of (B, A)"""
    payload, keys, counts, ref_off, rs, rt = _zipf_model(ctx, 10000000, 3, 12, thr=20)
    a, b, c, _ = ctx.cooc_resident(threshold=0)
    ntok = np.array([len(key_tokens(k)) for k in keys], dtype=np.int64)
    pid = np.repeat(np.arange(len(keys)), np.diff(ref_off.astype(np.int64)))
    s, t, n = rs.astype(np.int64), rt.astype(np.int64), ntok[pid]
    order = np.lexsort((t, s))
    s, t, n = s[order], t[order], n[order]
    # per occurrence (s, t, n): B's of its sentence that end before t - 1 or start after t + n, counted by binary search over the sentence's
    # starts and ends (both sorted per sentence)
    ends = s * (1 << 20) + t + n
    order_e = np.argsort(ends, kind="stable")
    ends_sorted = ends[order_e]
    starts = s * (1 << 20) + t
    before = np.searchsorted(ends_sorted, s * (1 << 20) + t, side="left") - np.searchsorted(ends_sorted, s * (1 << 20), side="left")
    after = np.searchsorted(starts, s * (1 << 20) + (1 << 20), side="left") - np.searchsorted(starts, starts + n, side="right")
    total = int(before.sum() + after.sum())
    assert int(c.astype(np.int64).sum()) == total
    P = len(keys)
    k1, k2 = a.astype(np.int64) * P + b, b.astype(np.int64) * P + a  # (A, B) and, for the same row, (B, A)
    o1, o2 = np.argsort(k1, kind="stable"), np.argsort(k2, kind="stable")
    assert np.array_equal(k1[o1], k2[o2]) and np.array_equal(c[o1], c[o2])


# ---- the CLI ---------------------------------------------------------------------------------------------------------------------------
def _parse(out, header):
    lines = out.splitlines()
    assert lines[0] == header
    return [ln.split("\t") for ln in lines[1:]]


def test_cli_builds_and_prints_cooc(tmp_path):
    data, cls = os.path.join(GOLDEN, "hamlet.v2.colibri.dat"), os.path.join(GOLDEN, "hamlet.colibri.cls")
    model = os.path.join(COOC, "hamlet.v2.is.colibri.patternmodel")
    want = load_fixture("hamlet.v2", "is", 2)
    for args in (["-i", model, "-f", data], ["-f", data, "-s", "-t", "2", "-l", "4"]):  # loaded; built (the same model: the reference's own)
        out = subprocess.run([CLI] + args + ["-c", cls, "-C", "2.7"], capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        rows = _parse(out.stdout, "Pattern1\tPattern2\tCooc")
        assert len(rows) == len(want)
        assert sorted(int(r[2]) for r in rows) == sorted(want.values())
        assert [int(r[2]) for r in rows] == sorted((int(r[2]) for r in rows), reverse=True)
        out = subprocess.run([CLI] + args + ["-c", cls, "-Y", "-0.3"], capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        rows = _parse(out.stdout, "Pattern1\tPattern2\tNPMI")
        counts, refs = load_model("hamlet.v2", "is")
        npmi = npmi_rows(counts, load_fixture("hamlet.v2", "is", 0), -0.3)
        assert len(rows) == len(npmi) and rows
        got = sorted(float(r[2]) for r in rows)
        assert got == pytest.approx(sorted(float(f"{v:.6g}") for v in npmi.values()), rel=1e-5)


def test_cli_unindexed_cooc_prints_nothing():
    out = subprocess.run([CLI, "-f", os.path.join(GOLDEN, "hamlet.v2.colibri.dat"), "-c", os.path.join(GOLDEN, "hamlet.colibri.cls"), "-u", "-t", "2", "-C", "2"],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout == ""


def test_cli_refuses_flexgram_models(tmp_path):
    model = str(tmp_path / "flex.colibri.patternmodel")
    data, cls = os.path.join(GOLDEN, "hamlet.v2.colibri.dat"), os.path.join(GOLDEN, "hamlet.colibri.cls")
    out = subprocess.run([CLI, "-f", data, "-s", "-T", "1", "-t", "2", "-l", "4", "-F", "S", "-o", model], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    out = subprocess.run([CLI, "-i", model, "-f", data, "-c", cls, "-C", "2"], capture_output=True, text=True)
    assert out.returncode != 0 and "flexgram" in out.stderr, out.stderr


def test_cxx_face_computecooc_and_computenpmi(tmp_path):
    """the reference's computecooc(coocmap, threshold) / computenpmi(coocmap, threshold) of the C++ face, on a loaded model"""
    out = str(tmp_path / "rows.txt")
    model = os.path.join(COOC, "edge.is.colibri.patternmodel")
    p = subprocess.run([os.path.join(os.path.dirname(CLI), "host_selftest"), "computecooc", model, os.path.join(GOLDEN, "edge.colibri.dat"), "2", out],
                       capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.startswith("OK"), p.stdout + p.stderr
    got = {}
    for ln in open(out).read().splitlines():
        a, b, c = ln.split("\t")
        got[(bytes.fromhex(a), bytes.fromhex(b))] = int(c)
    assert got == load_fixture("edge", "is", 2)
    counts, _ = load_model("edge", "is")
    assert int(p.stdout.split()[1]) == len(npmi_rows(counts, load_fixture("edge", "is", 0), -1.0))
