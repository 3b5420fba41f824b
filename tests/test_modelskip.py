"""Skipgrams of a loaded indexed model, the parts that need no GPU: the plain restatement of
IndexedPatternModel::trainskipgrams against the fixtures the reserved reference left (tests/golden/modelskip/) and against the direct -s
builds tests/golden/ already holds; the helper that installs a device answer in a model, under the sanitizers; the C++ face over the
stand-in device layer, which has no such entry point and must say so."""
import os
import subprocess

import pytest

import modelskip_models as mm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sorted(mm.cases())


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reserved_reference(name):
    c, model, want, err = mm.fixture(name)
    log, has, types = mm.restate(model, **mm.case_options(c))
    assert model == want  # patterns, counts (the lists' lengths) and the sorted lists
    assert all(len(set(refs)) == len(refs) for refs in model.values())  # two sources of one skipgram never share a reference
    assert log == c["orders"]
    assert has == c["hasskipgrams"]
    assert len(model) == c["patterns"]
    assert sum(1 for k in model if mm.GAP in k) == c["skipgrams"] == len(types)
    assert mm.progress_lines(log) == err  # D1: `total kept: 4294967075`, the reference's unsigned arithmetic


def test_total_kept_wraps_as_the_reference_prints_it():
    assert mm.progress_lines([[3, 238, 459, 0], [4, 32, 210, 0]])[2] == " Found 238 skipgrams...pruned 459...total kept: 4294967075"
    assert mm.progress_lines([[3, 12, 0, 10]])[2] == " Found 12 skipgrams...pruned 0 plus 10 extra skipgrams.....total kept: 2"
    assert mm.progress_lines([[3, 0, 0, 0]])[1:] == ["Counting 3-skipgrams", " None found"]


@pytest.mark.parametrize("igold,isgold,opts", mm.DIRECT, ids=[d[1] for d in mm.DIRECT])
def test_restatement_reproduces_the_direct_builds(igold, isgold, opts):
    model, want = mm.direct_pair(igold, isgold)
    log, has, _ = mm.restate(model, **opts)
    assert has and model == want
    assert all(pruned == 0 for _, _, pruned, _ in log)  # a model trained with the same t has nothing below it


def test_a1_equals_its_direct_build():
    c, model, want, _ = mm.fixture("A1")
    assert want == mm.load_rows(os.path.join(mm.GOLDEN, c["direct"]))


def test_gap_masks_are_the_recorded_ones():
    assert mm.gap_masks(3, 3) == [0b010]
    assert mm.gap_masks(5, 3) == [0b00010, 0b00100, 0b00110, 0b01000, 0b01010, 0b01100, 0b01110]
    assert 0b01010 not in mm.gap_masks(5, 1) and len(mm.gap_masks(5, 1)) == 6  # n - 2 >= maxskips: two gaps are one too many
    assert len(mm.gap_masks(5, 2)) == 7
    assert mm.gap_masks(4, 3) == [0b0010, 0b0100, 0b0110]  # n - 2 < maxskips: no limit
    assert len(mm.gap_masks(6, 1)) == 10 and len(mm.gap_masks(6, 2)) == 15


# ---- the helper that installs an answer (host/include/skipgram_merge.h), stand-alone and under the sanitizers ---------------------------------------
def test_skipgram_merge_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "skipgram_merge_check")
    inc = os.path.join(ROOT, "colibri-core_amd", "host", "include")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + inc,
                           os.path.join(ROOT, "tests", "skipgram_merge_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "skipgram_merge ok" in r.stdout


# ---- the C++ face over the stand-in device layer: the entry point is missing there and the call must say so ---------------------------------------
def test_mock_cli_names_the_missing_entry_point(tmp_path):
    mock = os.path.join(ROOT, "tests", "standin", "bin", "colibri-patternmodeller-mock")  # (absent: the stand-in no longer links, which is what this test is about)
    r = subprocess.run([mock, "-i", os.path.join(mm.FIXTURES, "hamlet.v2.i.t2l5.patternmodel"), "-f", os.path.join(mm.GOLDEN, "hamlet.v2.colibri.dat"), "-s", "-t", "2", "-l", "5",
                        "-o", str(tmp_path / "out.patternmodel")], capture_output=True, text=True)
    assert r.returncode == 1, r.stderr
    assert "colibri_modelskip" in r.stderr
    assert not os.path.exists(tmp_path / "out.patternmodel")
