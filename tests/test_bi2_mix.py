"""The radix engine's key mix and bin arithmetic without a device: csrc/bi2_mix.hpp compiled for the host (tests/bi2_mix_check.cpp: the mix is a
bijection of the K-bit integers — every value for K <= 24, inverted round trips beyond —, and its two product forms agree), the numpy restatement of
tests/bin_models.py pinned to the C++ on the vectors the check program prints, and the corpus builders pinned to the oracle: a corpus built to hold
D distinct bigrams and S survivors in one final bin trains to exactly the counts it was asked for. tests/test_gpu_bin_edges.py holds the device to
these corpora."""
import os
import subprocess

import numpy as np
import pytest

import bin_models as bm
from conftest import ROOT


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("bi2_mix") / "bi2_mix_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "colibri-core_amd", "csrc"), os.path.join(ROOT, "tests", "bi2_mix_check.cpp"), "-o", str(exe)])
    return str(exe)


def test_the_mix_is_a_bijection(check_exe):
    """every K-bit value for K = 17 .. 24 (range, no repeated image), 10^6 inverted round trips for each K = 25 .. 56, the edge inputs of seven K, both product forms"""
    p = subprocess.run([check_exe], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:]
    checked, mismatches = (int(x) for x in p.stdout.split()[1::2][-2:])
    assert mismatches == 0 and checked > sum(1 << K for K in range(17, 25)) + 32 * 10 ** 6, p.stdout[-500:]


@pytest.fixture(scope="module")
def vectors(check_exe):
    p = subprocess.run([check_exe, "vectors"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0
    rows = [line.split() for line in p.stdout.splitlines()]
    return [r for r in rows if r[0] == "M"], [r for r in rows if r[0] == "B"]


def test_python_mix_equals_the_cpp(vectors):
    mixes, _ = vectors
    assert len(mixes) >= 10 ** 4 and {int(r[1]) for r in mixes} == {17, 18, 24, 28, 34, 42, 48}
    for K in sorted({int(r[1]) for r in mixes}):
        x = np.array([int(r[2]) for r in mixes if int(r[1]) == K], dtype=np.uint64)
        y = np.array([int(r[3]) for r in mixes if int(r[1]) == K], dtype=np.uint64)
        assert (bm.mix(x, K) == y).all(), K
        assert (bm.unmix(y, K) == x).all(), K
        assert bm.mix(int(x[-1]), K) == int(y[-1]) and bm.unmix(int(y[-1]), K) == int(x[-1])  # (the scalar form)


def test_python_bucket_equals_the_cpp(vectors):
    _, buckets = vectors
    assert len(buckets) >= 3000 and {int(r[1]) for r in buckets} == {6, 7, 8}
    for lgb in (6, 7, 8):
        key = np.array([int(r[2]) for r in buckets if int(r[1]) == lgb], dtype=np.uint64)
        want = np.array([int(r[3]) for r in buckets if int(r[1]) == lgb], dtype=np.uint64)
        assert (bm.bucket(key, lgb) == want).all(), lgb
        assert bm.bucket(int(key[-1]), lgb) == int(want[-1])


def test_the_plan_arithmetic():
    """the restated constants at the values the issue's cases rest on"""
    assert [bm.clsbits(c) for c in (1, 63, 64, 4095, 4096, (1 << 21) - 1)] == [1, 6, 7, 12, 13, 21]
    assert [bm.order2_kbits(cb) for cb in (6, 8, 9, 12, 21)] == [17, 17, 18, 24, 42]
    assert [bm.bshift(r, 24) for r in (0, 8 * 256 * 700, 8 * 256 * 700 + 1, 10 ** 8)] == [6, 6, 5, 0]
    assert bm.bshift(0, 44) == 4 and bm.bshift(0, 48) == 0
    assert [bm.table_slots(t) for t in (1, 171, 172, 341, 342, 100000)] == [256, 256, 512, 512, 1024, 1024]
    assert [bm.table_lgb(t) for t in (171, 172, 342)] == [6, 7, 8]
    assert [bm.wcap(n) for n in (0, 8533, 8534, 17067)] == [4096, 4096, 4098, 4100]
    assert bm.region(10000) == 4096 and bm.region(16 * 1024 * 1024) == 2 * (16 * 1024 * 1024 + 1) // 1024
    assert [bm.pshift(n) for n in (1, 4096 * 1024 - 1, 4096 * 1024)] == [12, 12, 13]


def test_keys_in_bin_land_in_their_bin_and_bucket():
    for fbin in ((0, 0), (255, 7), (100, 3)):
        keys = bm.keys_in_bin(fbin, 901)
        assert len(set(keys)) == 901 and all(64 <= a <= 4095 and 64 <= b <= 4095 for a, b in keys)
        a, b = (np.array(v, dtype=np.uint64) for v in zip(*keys))
        A, B = bm.final_bin(a, b)
        assert (A == fbin[0]).all() and (B == fbin[1]).all()
        assert len(set(bm.inbin_key(a, b).tolist())) == 901  # distinct bigrams of a bin have distinct table keys
        for lgb in (6, 7, 8):
            for bk in (bm.full_bucket(fbin, lgb, 17), (1 << lgb) - 1):
                ks = bm.keys_in_bin(fbin, 17, in_bucket=bk, lgb=lgb)
                assert all(bm.bucket(bm.inbin_key(a, b), lgb) == bk and bm.final_bin(a, b) == fbin for a, b in ks)
    # every final bin of a small order holds far more bigrams of classes 64 .. 4095 than a test needs
    y = np.arange(1 << 24, dtype=np.uint64)
    x = bm.unmix(y, 24)
    ok = ((x >> np.uint64(12)) >= 64) & ((x & np.uint64(4095)) >= 64)
    per_bin = np.bincount((y[ok] >> np.uint64(13)).astype(np.int64), minlength=2048)
    assert per_bin.min() >= 7000 and per_bin.size == 2048


@pytest.mark.parametrize("name", sorted(bm.cpu_cases()))
def test_builders_mean_what_they_say(name):
    """members of every corpus family of tests/test_gpu_bin_edges.py: trained by the oracle, a corpus gives exactly the counts its builder was asked for, and
    (Case.check, inside the builder) it holds the records, head windows and bin contents its case names"""
    import oracle
    build, maxlength = bm.cpu_cases()[name]
    corpus = build().corpus
    want = oracle.train(corpus.payload, corpus.mintokens, maxlength)
    assert want.counts == corpus.model(maxlength)
    assert want.counts, "an empty model says nothing"
