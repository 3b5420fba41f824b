"""The chained orders' step tables without a device: csrc/chain_step.hpp compiled for the host (tests/chain_step_check.cpp: an entry gives back its pairs and its
bucket, and the blocks' runs of consecutive entries cover a table exactly once), and the corpora of tests/test_gpu_chain_bits.py held to what they are built for
(tests/chain_bits_models.py: Edges.check, inside the builder) and to the oracle."""
import os
import subprocess

import pytest

import chain_bits_models as cb
from conftest import ROOT


def test_step_entries_and_runs(tmp_path):
    exe = tmp_path / "chain_step_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "colibri-core_amd", "csrc"), os.path.join(ROOT, "tests", "chain_step_check.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:]
    checked, mismatches = (int(x) for x in p.stdout.split()[1::2][-2:])
    assert mismatches == 0 and checked > 2049 * 1024


@pytest.mark.parametrize("last", [545, 577, 609])
def test_the_corpora_hold_their_cases(last):
    """the builder's own assertions (every edge case occurs), the slice lengths modulo four over the three corpora, and the oracle's model of the corpus"""
    import oracle
    case = cb.edges(last)
    assert case.slice_words[0] % 4 == {545: 2, 577: 3, 609: 0}[last] and case.slice_words[1] % 4 == 1
    want = oracle.train(case.corpus.payload, 2, 5)
    assert want.counts == case.corpus.model(5) and want.maxn == 5
