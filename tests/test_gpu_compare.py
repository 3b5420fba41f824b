"""Log-likelihood model comparison on the device (colibri_compare; colibri-comparemodels and the C++ face), against the reference's output
(tests/golden/compare/) and the restatement in test_compare.py, under the precision rule there: ll within 1e-9 * max(1, |ll|), every other
column and the pattern text exact, the order the reference's except among rows whose ll lie within that tolerance of each other."""
import math
import os
import random
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from test_compare import (CASES, CLI, CMP, category, compare, case_models, decode, direct_lines, expected, golden, group_totals, key_tokens, load,
                          numeric_equal, read_classes, sorted_text, split_direct)

pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "colibri-core_amd", "bin")
TOL = 1e-9


@pytest.fixture(scope="module")
def ctx():
    from colibri_amd import capi
    with capi.Context(0) as c:
        yield c


def arrays(tokens, model):
    keys = list(model)
    off = np.zeros(len(keys) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(k) for k in keys])
    kb = np.frombuffer(b"".join(keys) or b"\0", dtype=np.uint8)
    cnt = np.array([model[k] for k in keys] or [0], dtype=np.uint32)[: len(keys)]
    return keys, (off, kb, cnt, tokens)


def close(a, b):
    return abs(a - b) <= TOL * max(1.0, abs(b))


def check_device(ctx, models, conjunction):
    """ctx.compare against the restatement: rows, representatives, counts, group totals, ll, order"""
    flat = [arrays(t, m) for t, m in models]
    keys = [k for k, _ in flat]
    want = {k: (ll, obs) for k, ll, obs in compare(models, conjunction)}
    gts = [group_totals(m) for _, m in models]
    for sorted_ in (True, False):
        model, index, ll, obs, gt = ctx.compare([a for _, a in flat], conjunction=conjunction, sorted=sorted_)
        assert len(ll) == len(want)
        got = [keys[m][i] for m, i in zip(model.tolist(), index.tolist())]
        assert len(set(got)) == len(got) and set(got) == set(want)
        for r, k in enumerate(got):
            wll, wobs = want[k]
            first = next(j for j, (_, mm) in enumerate(models) if k in mm)
            assert model[r] == first  # the representative is the first occurrence
            assert obs[r].tolist() == wobs, k
            g = (category(k), len(key_tokens(k)))
            assert gt[r].tolist() == [0 if g[0] == 3 else gg.get(g, 0) & 0xFFFFFFFF for gg in gts]
            assert close(ll[r], wll), (k, ll[r], wll)
        if sorted_:
            for r in range(len(got) - 1):
                a, b = (-ll[r], got[r]), (-ll[r + 1], got[r + 1])
                assert a < b or close(ll[r], ll[r + 1]), (r, a, b)
                if ll[r] == ll[r + 1] or (ll[r] == 0 and ll[r + 1] == 0):
                    assert got[r] < got[r + 1]
        else:
            assert [(m, i) for m, i in zip(model.tolist(), index.tolist())] == sorted(zip(model.tolist(), index.tolist()))
    return len(want)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_device_matches_the_restatement(ctx, case):
    check_device(ctx, case_models(case), "-a" in case["opts"])


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_forced_hash_collisions_give_the_same_rows(ctx, case, monkeypatch):
    monkeypatch.setenv("COLIBRI_COMPARE_HASH_BITS", "3")  # eight hash values: identity is decided by the bytes alone
    check_device(ctx, case_models(case), "-a" in case["opts"])


def run_cli(args, env=None, timeout=300):
    r = subprocess.run([CLI] + args, capture_output=True, text=True, env=env, timeout=timeout)
    assert r.returncode == 0, r.stderr
    return r.stdout


def check_direct(got, want, nmodels):
    gh, gl = split_direct(got, nmodels)
    wh, wl = split_direct(want, nmodels)
    assert len(gl) == len(wl)
    def cols(lines):  # (text, counts, FREQ) -> the ll printed, as a multiset: two patterns may print as the same text
        out = {}
        for l in lines:
            f = l.split("\t")
            out.setdefault((f[0], tuple(f[2:])), []).append(float(f[1]))
        return {k: sorted(v) for k, v in out.items()}
    gm, wm = cols(gl), cols(wl)
    assert set(gm) == set(wm)
    for k, w in wm.items():
        for a, b in zip(gm[k], w):
            assert abs(a - b) <= TOL * max(1.0, abs(b)) + 1e-5 * abs(b), (k, a, b)


@pytest.mark.parametrize("hashbits", [None, "2"])
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_cli_matches_the_reference(case, hashbits):
    env = dict(os.environ)
    if hashbits:
        env["COLIBRI_COMPARE_HASH_BITS"] = hashbits
    args = ["-c", os.path.join(GOLDEN, case["cls"])] + case["opts"] + [os.path.join(CMP, m) for m in case["models"]]
    got, want = run_cli(args, env), golden(case)
    if "-d" in case["opts"]:
        check_direct(got, want, len(case["models"]))
    else:
        numeric_equal(got, want)


@pytest.mark.parametrize("opts", [["-S"], ["-S", "-a"], ["-S", "-d"]])
def test_cli_omit_skipgrams_against_the_restatement(opts):
    """(the reference's -S loses its place in the model file and prints garbage, so -S is held against the restatement)"""
    ms = ["hamlet.v2.20.us.colibri.patternmodel", "hamlet.v2.21.us.colibri.patternmodel"]
    case = {"models": ms, "opts": opts, "cls": "hamlet.colibri.cls"}
    models, rows, cls = expected(case)
    assert all(category(k) == 1 for _, m in models for k in m)
    got = run_cli(["-c", os.path.join(GOLDEN, "hamlet.colibri.cls")] + opts + [os.path.join(CMP, m) for m in ms])
    if "-d" in opts:
        _, gl = split_direct(got, 2)
        want = direct_lines(models, rows, cls)
        assert sorted(l.split("\t")[0] for l in gl) == sorted(l.split("\t")[0] for l in want)
    else:
        numeric_equal(got, sorted_text(models, rows, cls))


def test_end_to_end_classencode_patternmodeller_comparemodels(tmp_path):
    rng = random.Random(5)
    words = [f"w{j}" for j in range(60)]
    names = []
    for j, bias in enumerate((0, 10, 25)):
        lines = [" ".join(words[min(59, int(rng.paretovariate(1.2)) + bias - 1)] for _ in range(rng.randint(3, 12))) for _ in range(400)]
        p = tmp_path / f"part{j}.txt"
        p.write_text("\n".join(lines) + "\n")
        names.append(p.name)
    r = subprocess.run([os.path.join(BIN, "colibri-classencode"), "-o", "tmp"] + names, cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    pms = []
    for n in names:
        stem = n[:-4]
        r = subprocess.run([os.path.join(BIN, "colibri-patternmodeller"), "-f", stem + ".colibri.dat", "-o", stem + ".colibri.patternmodel", "-u", "-t", "2", "-l", "3"],
                           cwd=tmp_path, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        pms.append(str(tmp_path / (stem + ".colibri.patternmodel")))
    got = run_cli(["-c", str(tmp_path / "tmp.colibri.cls")] + pms)
    models = [load(p, []) for p in pms]
    cls = read_classes(str(tmp_path / "tmp.colibri.cls"))
    numeric_equal(got, sorted_text(models, compare(models), cls))
    got = run_cli(["-a", "-c", str(tmp_path / "tmp.colibri.cls")] + pms)
    numeric_equal(got, sorted_text(models, compare(models, True), cls))


def zipf_models(ctx, ntok, nmodels, seed, **train):
    """a Zipf corpus cut into nmodels sentence ranges, each trained on the device: [(tokens, {key: count})] and the flat arrays"""
    from colibri_amd import synth
    out = []
    for m in range(nmodels):
        payload = synth.zipf_corpus(ntok // nmodels, 20000, seed + m, phrases=True, header=False)
        ctx.upload(payload)
        st = ctx.train(**train)
        key_off, key_bytes, counts, _ = ctx.export_arrays()
        out.append((st.totaltokens, key_off, key_bytes, counts))
    return out


def as_dicts(flat):
    res = []
    for tokens, off, kb, cnt in flat:
        b, o = kb.tobytes(), off.tolist()
        res.append((tokens, {b[o[j]:o[j + 1]]: int(c) for j, c in enumerate(cnt.tolist())}))
    return res


@pytest.mark.parametrize("nmodels,train", [(2, dict(mintokens=2, maxlength=3)), (3, dict(mintokens=2, maxlength=3, indexed=1)),
                                            (4, dict(mintokens=2, maxlength=4, doskipgrams=1, indexed=1))])
def test_a_million_tokens_against_the_restatement(ctx, nmodels, train):
    models = as_dicts(zipf_models(ctx, 1_000_000, nmodels, 11, **train))
    for conj in (False, True):
        n = check_device(ctx, models, conj)
        assert n > 1000


def test_ten_million_tokens_invariants(ctx):
    flat = zipf_models(ctx, 10_000_000, 2, 21, mintokens=2, maxlength=4)
    models = as_dicts(flat)
    union = set().union(*[set(m) for _, m in models])
    inter = set(models[0][1]).intersection(*[set(m) for _, m in models[1:]])
    total = [t for t, _ in models]
    for conj, want in ((False, union), (True, inter)):
        model, index, ll, obs, _ = ctx.compare([(o, k, c, t) for t, o, k, c in flat], conjunction=conj)
        assert len(ll) == len(want)
        keys = [list(m) for _, m in models]
        got = [keys[m][i] for m, i in zip(model.tolist(), index.tolist())]
        assert set(got) == want
        assert np.all(-ll[:-1] <= -ll[1:] + TOL * np.maximum(1.0, np.abs(ll[1:])))
        for r in random.Random(3).sample(range(len(got)), min(10_000, len(got))):
            k = got[r]
            assert obs[r].tolist() == [m.get(k, 0) for _, m in models]
            from test_compare import loglikelihood
            assert close(ll[r], loglikelihood(obs[r].tolist(), total))
        distinct, scratch = ctx.compare_info()
        assert distinct == len(union) and scratch > 0


def test_eight_models(ctx):
    models = as_dicts(zipf_models(ctx, 800_000, 8, 31, mintokens=2, maxlength=3))
    assert check_device(ctx, models, False) > 1000
    check_device(ctx, models, True)


def test_refuses_a_model_over_int_max_tokens(ctx):
    from colibri_amd import capi
    _, a = arrays(10, {b"\x05": 1})
    with pytest.raises(Exception):
        ctx.compare([a, (a[0], a[1], a[2], 2 ** 31)])
