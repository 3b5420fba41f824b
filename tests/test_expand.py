"""Expanding a loaded model on further corpus data (-e without -E): the plain restatement (tests/expand_models.py) against the real reference's results
(tests/golden/expand/, see its README.md). No device: tests/test_gpu_expand.py holds the device, the C++ face and the CLI to the same goldens."""
import functools
import os
import subprocess

import pytest

import expand_models as em
from conftest import GOLDEN, ROOT

EXPAND = os.path.join(GOLDEN, "expand")

# golden file -> (first corpus, [(further corpus, firstsentence), ...], MAXLENGTH, MINTOKENS, indexed)
CASES = {
    "zipf20k+phrases15k.u.l5t2": ("zipf20k", [("phrases15k", 1)], 5, 2, False),
    "zipf20k+phrases15k.u.l5t3": ("zipf20k", [("phrases15k", 1)], 5, 3, False),
    "phrases15k+zipf20k.u.l5t2": ("phrases15k", [("zipf20k", 1)], 5, 2, False),
    "edge+shortlines.u.l4t2": ("edge", [("shortlines", 1)], 4, 2, False),
    "hamlet.v2+hamlet.v2.u.l5t2": ("hamlet.v2", [("hamlet.v2", 1)], 5, 2, False),
    "edge+shortlines.i.l4t2.e1000": ("edge", [("shortlines", 1000)], 4, 2, True),
    "hamlet.v2+hamlet.v2.i.l5t2.e100001": ("hamlet.v2", [("hamlet.v2", 100001)], 5, 2, True),
    "hamlet.v2+hamlet.v2.i.l5t2.e1": ("hamlet.v2", [("hamlet.v2", 1)], 5, 2, True),
    "edge+shortlines+hamlet.v2.u.l4t2": ("edge", [("shortlines", 1000), ("hamlet.v2", 5000)], 4, 2, False),
    "edge+shortlines+hamlet.v2.i.l4t2": ("edge", [("shortlines", 1000), ("hamlet.v2", 5000)], 4, 2, True),
}


@functools.lru_cache(maxsize=None)
def payload(name):
    data = open(os.path.join(GOLDEN, name + ".colibri.dat"), "rb").read()
    assert data[:2] == b"\xa2\x02"
    return data[2:]


@functools.lru_cache(maxsize=None)
def first_model(name, l, t, indexed):
    return em.train(payload(name), t, l, indexed=indexed)


def step(m, corpus, first, l, t, indexed):
    return em.expand(m.refs if indexed else m.counts, payload(corpus), t, l, indexed=indexed, firstsentence=first, tokens=m.tokens, types=m.types, maxn=m.maxn, minn=m.minn)


@functools.lru_cache(maxsize=None)
def restated(tag):
    first, more, l, t, indexed = CASES[tag]
    m = first_model(first, l, t, indexed)
    for corpus, fs in more:
        m = step(m, corpus, fs, l, t, indexed)
    return m


def golden(tag):
    return em.parse_golden(open(os.path.join(EXPAND, tag + ".txt")).read())


def test_the_first_models_are_the_oracles():
    """the restatement started from the empty model is an ordinary train(): the C oracle's model, totals included"""
    import oracle
    for name, l, t in (("zipf20k", 5, 2), ("edge", 4, 2), ("hamlet.v2", 5, 2)):
        want = oracle.train(payload(name), t, l, indexed=True)
        got = first_model(name, l, t, True)
        assert (got.counts, got.refs, got.tokens, got.types) == (want.counts, want.refs, want.tokens, want.types), name


@pytest.mark.parametrize("tag", list(CASES))
def test_restatement_equals_the_reference(tag):
    head, counts, refs = golden(tag)
    m = restated(tag)
    assert (m.tokens, m.types, m.maxn, m.minn) == (head["tokens"], head["types"], head["maxn"], head["minn"])
    assert m.counts == counts
    if CASES[tag][4]:
        assert m.refs == refs


@pytest.mark.parametrize("tag", [t for t in CASES if len(CASES[t][1]) == 1 and not CASES[t][4]])
def test_every_pair_has_rows_a_naive_sum_gets_wrong(tag):
    """training the second corpus alone and adding the two models gives other counts: a device that did that could not pass by accident"""
    first, ((corpus, _),), l, t, _ = CASES[tag]
    naive = em.naive_sum(first_model(first, l, t, False).counts, em.train(payload(corpus), t, l).counts)
    _, counts, _ = golden(tag)
    wrong = [k for k in counts if naive.get(k) != counts[k]]
    assert wrong, tag
    if tag == "zipf20k+phrases15k.u.l5t2":
        assert len(counts) == 6916 and len(wrong) == 659


def test_the_hamlet_pair_stops_at_order_4():
    """expanded on its own corpus the model creates nothing at order 4: the run stops there, before the prune, and the loaded 5-grams keep their counts"""
    m = restated("hamlet.v2+hamlet.v2.u.l5t2")
    loaded = first_model("hamlet.v2", 5, 2, False)
    assert m.stop == 4 and m.maxn == 5 and m.found[4] == 0 and len(m.counts) == 102
    five = [k for k in loaded.counts if em.ntokens(k) == 5]
    assert len(five) == 9 and all(m.counts[k] == loaded.counts[k] for k in five)
    four = [k for k in loaded.counts if em.ntokens(k) == 4]
    assert four and all(m.counts[k] == 2 * loaded.counts[k] for k in four)


def test_expand_merge_under_the_sanitizers(tmp_path):
    """host/include/expand_merge.h (what train_expand does to the host's map with a seeded run's answer) on hand-made inputs: sums replace counts, references
    join in ascending order, created rows enter, the seeds that do not stay leave, broken answers are refused with the map untouched; ordered and unordered
    maps (tests/expand_merge_check.cpp holds the cases)"""
    exe = tmp_path / "expand_merge_check"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "colibri-core_amd", "host", "include"),
                           os.path.join(ROOT, "tests", "expand_merge_check.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.split()[0] == "checked" and out.stdout.split()[3] == "0"


def test_a_device_layer_without_the_seed_entry_points_refuses_loudly():
    """the C++ face refers to colibri_set_seed / colibri_seed_fetch weakly: over a device layer that lacks them (the CPU stand-in of tests/standin) it links, and
    expanding a loaded model ends with a message and a failure status instead of a model"""
    cli = os.path.join(ROOT, "tests", "standin", "bin", "colibri-patternmodeller-mock")
    out = subprocess.run([cli, "-i", os.path.join(GOLDEN, "continued.zipf20k.u.t3l2.patternmodel"), "-f", os.path.join(GOLDEN, "zipf20k.colibri.dat"), "-e", "1000", "-u", "-l", "3"],
                         capture_output=True, text=True)
    assert out.returncode == 1 and "has no colibri_set_seed" in out.stderr, out.stderr
