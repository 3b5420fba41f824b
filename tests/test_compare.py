"""Log-likelihood model comparison (colibri-comparemodels; reference src/comparemodels.cpp, comparemodels_loglikelihood in src/patternmodel.cpp:22-171).

CPU part: a restatement of the reference's specification — the rows (union, or with -a the patterns every model holds), the ll expression
in its order of evaluation, the sorted order (-ll, key bytes), FREQ = count / (double)(the model's total of the pattern's (category, size)
group) and the -d text — checked against the real reference's output on every fixture case (tests/golden/compare/, see the README there);
the CLI's refusals that need no device; the C ABI symbols. The GPU part (tests/test_gpu_compare.py) holds the device and the CLI against
this restatement and the fixtures."""
import gzip
import json
import math
import os
import subprocess

import pytest

from conftest import GOLDEN, ROOT
from test_host_face import parse_model

CMP = os.path.join(GOLDEN, "compare")
CLI = os.path.join(ROOT, "colibri-core_amd", "bin", "colibri-comparemodels")
CASES = json.load(open(os.path.join(CMP, "cases.json")))
HEADER = "PATTERN\tLOGLIKELIHOOD"


def key_tokens(key):
    out, start = [], 0
    for j, b in enumerate(key):
        if b < 128:
            out.append(key[start:j + 1])
            start = j + 1
    return out


def category(key):
    """colibri_host::category_of: the first token that is the skip class (3) -> skipgram (2), the flex class (4) -> flexgram (3), else n-gram (1)"""
    for t in key_tokens(key):
        if t == b"\x03":
            return 2
        if t == b"\x04":
            return 3
    return 1


def read_classes(path):
    cls = {2: "{?}", 3: "{*}", 4: "{**}", 1: "{|}"}
    for line in open(path, encoding="utf-8"):
        line = line.rstrip("\n")
        if "\t" in line:
            k, w = line.split("\t", 1)
            cls[int(k)] = w
    return cls


def decode(key, cls):
    words = []
    for t in key_tokens(key):
        v = 0
        for j, b in enumerate(t):
            v |= (b & 127) << (7 * j)
        words.append(cls.get(v, "{?}"))
    return " ".join(words)


def fmt(x):
    """iostream's default double format (6 significant digits); glibc prints the x86 default NaN (0.0 / 0.0) as -nan"""
    if math.isnan(x):
        return "-nan" if math.copysign(1.0, x) < 0 else "nan"
    if math.isinf(x):
        return "inf" if x > 0 else "-inf"
    return f"{x:g}"


def load(path, opts):
    """PatternModel<uint32_t>(file, options) with the CLI's -l / -m / -S / -F: (tokens, {key: count} in file order)"""
    _, tokens, _, counts, _ = parse_model(path)
    maxlen = int(opts[opts.index("-l") + 1]) if "-l" in opts else 100
    minlen = int(opts[opts.index("-m") + 1]) if "-m" in opts else 1
    out = {}
    for k, c in counts.items():
        cat = category(k)
        if ("-S" in opts and cat == 2) or ("-F" in opts and cat == 3):
            continue
        if not minlen <= len(key_tokens(k)) <= maxlen:
            continue
        out[k] = c
    return tokens, out


def loglikelihood(observed, total):
    """the reference's expression, its integer types and its order of evaluation (patternmodel.h:114-150)"""
    n_sum, o_sum = sum(total), sum(observed)
    expected = [math.exp((math.log(n) if n > 0 else -math.inf) + (math.log(o_sum) if o_sum > 0 else -math.inf) - (math.log(n_sum) if n_sum > 0 else -math.inf))
                for n in total]
    ll = 0.0
    for o, e in zip(observed, expected):
        if o > 0:
            ll = ll + o * (math.log(o / e) if e > 0 else math.inf)
    ll = ll * 2
    return 0.0 if math.isnan(ll) else ll


def group_totals(model):
    """per (category, tokens): the occurrences of the model's patterns of that group (a flexgram adds to none that is asked)"""
    tot = {}
    for k, c in model.items():
        cat = category(k)
        if cat != 3:
            g = (cat, len(key_tokens(k)))
            tot[g] = tot.get(g, 0) + c
    return tot


def compare(models, conjunction=False):
    """rows (key, ll, observed[]) of the comparison: union in first-occurrence order (model, then file order), or the conjunction"""
    seen, rows = set(), []
    total = [t for t, _ in models]
    for _, m in models:
        for k in m:
            if k in seen:
                continue
            seen.add(k)
            obs = [mm.get(k, 0) for _, mm in models]
            if conjunction and 0 in obs:
                continue
            rows.append((k, loglikelihood(obs, total), obs))
    return rows


def sorted_rows(rows):
    return sorted(rows, key=lambda r: (-r[1], r[0]))


def freq(o, t):
    if t == 0:
        return "-nan" if o == 0 else "inf"
    return fmt(o / t)


def sorted_text(models, rows, cls):
    gts = [group_totals(m) for _, m in models]
    out = [HEADER + "".join(f"\tOCC_{i}\tFREQ_{i}" for i in range(len(models)))]
    for k, ll, obs in sorted_rows(rows):
        g = (category(k), len(key_tokens(k)))
        cols = "".join(f"\t{o}\t{freq(o, 0 if g[0] == 3 else gt.get(g, 0) & 0xFFFFFFFF)}" for o, gt in zip(obs, gts))
        out.append(f"{decode(k, cls)}\t{fmt(-(-ll))}{cols}")
    return "\n".join(out) + "\n"


def direct_lines(models, rows, cls):
    total = [t for t, _ in models]
    out = []
    for k, ll, obs in rows:
        cols = "".join(f"\t{o}\t{(o // t) if t > 0 else 0}" for o, t in zip(obs, total))
        out.append(f"{decode(k, cls)}\t{fmt(ll)}{cols}")
    return out


def split_direct(text, nmodels):
    """-d text: the header has no newline, so the first row follows it on its line; -> (header, row lines)"""
    head = HEADER + "".join(f"\tOCC_{i}\tFREQ_{i}" for i in range(nmodels))
    assert text.startswith(head), text[:200]
    body = text[len(head):]
    return head, [l for l in body.split("\n") if l]


def golden(case):
    with gzip.open(os.path.join(CMP, case["golden"]), "rb") as f:
        return f.read().decode("utf-8")


def case_models(case):
    return [load(os.path.join(CMP, m), case["opts"]) for m in case["models"]]


def expected(case):
    models = case_models(case)
    rows = compare(models, "-a" in case["opts"])
    cls = read_classes(os.path.join(GOLDEN, case["cls"]))
    return models, rows, cls


def numeric_equal(got, want, tol=1e-9):
    """two outputs of the same rows: pattern text and every column other than LOGLIKELIHOOD byte-identical, LOGLIKELIHOOD within tol * max(1, |ll|),
    the order equal except among rows whose ll lie within that tolerance of each other"""
    g, w = got.rstrip("\n").split("\n"), want.rstrip("\n").split("\n")
    assert len(g) == len(w), (len(g), len(w))
    assert g[0] == w[0]
    gr = [l.split("\t") for l in g[1:]]
    wr = [l.split("\t") for l in w[1:]]
    def close(a, b):  # (both sides are printed to 6 significant digits: one unit of the last digit apart is the same value)
        a, b = float(a), float(b)
        return abs(a - b) <= tol * max(1.0, abs(b)) + 1e-5 * abs(b)
    # the rows as a multiset (two patterns may print as the same text); position by position the ll agree, so rows can only trade places
    # with rows of an ll within the tolerance; where a row's text and counts are unique, its own ll agrees
    assert sorted((r[0], r[2:]) for r in gr) == sorted((r[0], r[2:]) for r in wr)
    for a, b in zip(gr, wr):
        assert a[1] == b[1] or close(a[1], b[1]), (a, b)
    seen = {}
    for r in wr:
        seen.setdefault((r[0], tuple(r[2:])), []).append(r[1])
    for r in gr:
        v = seen[(r[0], tuple(r[2:]))]
        if len(v) == 1:
            assert r[1] == v[0] or close(r[1], v[0]), (r, v)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_restatement_matches_the_reference(case):
    models, rows, cls = expected(case)
    want = golden(case)
    if "-d" in case["opts"]:
        head, lines = split_direct(want, len(models))
        assert sorted(lines) == sorted(direct_lines(models, rows, cls))
    else:
        assert sorted_text(models, rows, cls) == want


def test_fixtures_cover_the_cases():
    names = {c["name"] for c in CASES}
    opts = [c["opts"] for c in CASES]
    assert any(len(c["models"]) == 2 for c in CASES) and any(len(c["models"]) == 3 for c in CASES)
    for flag in ("-a", "-l", "-m", "-d"):
        assert any(flag in o for o in opts), flag
    assert "zipf20k.same" in names
    same = golden(next(c for c in CASES if c["name"] == "zipf20k.same"))
    assert all(abs(float(l.split("\t")[1])) < 1e-9 for l in same.split("\n")[1:] if l)  # identical models: every ll 0 up to residues of log / exp
    empty = golden(next(c for c in CASES if c["name"] == "zipf20k.2.u_l1_m2"))
    assert "\t0\t-nan" in empty  # a model empty after filtering: 0 / 0
    kinds = {parse_model(os.path.join(CMP, m))[0] for c in CASES for m in c["models"]}
    assert kinds == {10, 20}
    assert any(category(k) == 2 for c in CASES for m in c["models"] for k in parse_model(os.path.join(CMP, m))[3])


def test_identical_models_order_by_key_bytes():
    t, m = load(os.path.join(CMP, CASES[0]["models"][0]), [])
    rows = compare([(t, m), (t, m)])
    assert all(abs(r[1]) < 1e-9 for r in rows)
    exact = [(k, 0.0, o) for k, _, o in rows]  # with the residues folded to 0, the order is the key bytes' alone
    assert [r[0] for r in sorted_rows(exact)] == sorted(m)


def test_loglikelihood_hand_worked():
    # o = (10, 0), n = (100, 100): e = (5, 5), ll = 2 * 10 * log(2)
    assert loglikelihood([10, 0], [100, 100]) == 2 * (10 * math.log(10 / math.exp(math.log(100) + math.log(10) - math.log(200))))
    assert abs(loglikelihood([10, 0], [100, 100]) - 20 * math.log(2)) < 1e-12
    assert loglikelihood([0, 0], [100, 100]) == 0.0  # NaN -> 0
    assert sorted_rows([(b"b", 1.0, []), (b"a", 1.0, []), (b"ab", 1.0, []), (b"c", 2.0, [])])[0][0] == b"c"
    assert [r[0] for r in sorted_rows([(b"b", 1.0, []), (b"ab", 1.0, []), (b"a", 1.0, [])])] == [b"a", b"ab", b"b"]  # a proper prefix first


def test_cli_refusals_need_no_device():
    models = [os.path.join(CMP, m) for m in CASES[0]["models"]]
    cls = os.path.join(GOLDEN, CASES[0]["cls"])
    r = subprocess.run([CLI] + models, capture_output=True, text=True)
    assert r.returncode == 2 and "No class file specified" in r.stderr
    r = subprocess.run([CLI, "-c", cls, models[0]], capture_output=True, text=True)
    assert r.returncode == 2 and "Need at least two models" in r.stderr
    r = subprocess.run([CLI, "-N", "-c", cls] + models, capture_output=True, text=True)
    assert r.returncode == 2 and "-N" in r.stderr and r.stdout == ""
    r = subprocess.run([CLI, "-h"], capture_output=True, text=True)
    assert r.returncode == 0 and "colibri-comparemodels" in r.stderr
    r = subprocess.run([CLI, "-Q", "-c", cls] + models, capture_output=True, text=True)
    assert r.returncode == 2


def test_abi_declares_the_compare_entry_points():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "colibri-core_amd", "pyhost"))
    from colibri_amd import capi
    hdr = open(os.path.join(ROOT, "include", "colibri_hip.h")).read()
    for name in ("colibri_compare", "colibri_compare_fetch", "colibri_compare_info"):
        assert name + "(" in hdr and name in capi.EXPORTED
    assert "COLIBRI_COMPARE_CONJUNCTION = 1, COLIBRI_COMPARE_UNSORTED = 2" in hdr
    assert (capi.COMPARE_CONJUNCTION, capi.COMPARE_UNSORTED) == (1, 2)
    assert "#define COLIBRI_ABI_VERSION 4 " in hdr
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "colibri-core_amd", "lib", "libcolibri_hip.so")], capture_output=True, text=True).stdout
    for name in ("colibri_compare", "colibri_compare_fetch", "colibri_compare_info"):
        assert f" T {name}\n" in nm
