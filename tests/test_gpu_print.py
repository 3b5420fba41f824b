"""The model text and histogram on the device (colibri_print_model / colibri_histogram; colibri-patternmodeller -P / -H under COLIBRI_PRINT /
COLIBRI_HISTOGRAM), against the restatement of test_print.py and the reference's text in tests/golden/views/. Every comparison is of bytes."""
import hashlib
import os
import random
import subprocess

import numpy as np
import pytest

from conftest import zipf_cached
from test_gpu_coverage import flat, varint
from test_print import case_arrays, histogram_rows, print_rows, read_classes
from test_views import CASES, CLI, GOLD, ROOT, VIEWS, golden

pytestmark = pytest.mark.gpu
LIB = os.path.join(ROOT, "colibri-core_amd", "lib")
HEADER = b"PATTERN\tCOUNT\tTOKENS\tCOVERAGE\tCATEGORY\tSIZE\tFREQUENCY"


@pytest.fixture(scope="module")
def ctx():
    from colibri_amd import capi
    with capi.Context(0) as c:
        yield c


def cli(args, **env):
    p = subprocess.run([CLI] + args, capture_output=True, env={**os.environ, **env}, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    return p.stdout, p.stderr.decode()


def same_rows(out, want):
    got_lines, want_lines = out.split(b"\n"), want.split(b"\n")
    assert got_lines[0] == want_lines[0]
    assert sorted(got_lines[1:]) == sorted(want_lines[1:])


# ---- the golden view cases through the CLI -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_cli_after_training(case):
    corpus, flags, cls = CASES[case]
    form = "resident" if "-s" in flags and "-u" not in flags else "uploaded"  # the trainings that leave their model in HBM: indexed with skipgrams
    args = ["-f", os.path.join(GOLD, f"{corpus}.colibri.dat"), "-c", os.path.join(GOLD, cls)] + flags
    out, err = cli(args + ["-P"], COLIBRI_PRINT="device")
    same_rows(out, golden(case, "print"))
    assert f"(print on the device: {form} model)" in err
    out, err = cli(args + ["-H"], COLIBRI_HISTOGRAM="device")
    assert out == golden(case, "histogram") and f"(histogram on the device: {form} model)" in err


@pytest.mark.parametrize("case", list(CASES))
def test_cli_on_a_loaded_model(case):
    args = ["-i", os.path.join(VIEWS, f"{case}.colibri.patternmodel"), "-c", os.path.join(GOLD, CASES[case][2])] + (["-u"] if "-u" in CASES[case][1] else [])
    out, err = cli(args + ["-P"], COLIBRI_PRINT="device")
    same_rows(out, golden(case, "print"))
    assert "(print on the device: uploaded model)" in err
    out, err = cli(args + ["-H"], COLIBRI_HISTOGRAM="device")
    assert out == golden(case, "histogram") and "(histogram on the device: uploaded model)" in err
    out, err = cli(args + ["-P", "-H"])  # auto: a model this small stays on the host
    assert "on the device" not in err


# ---- windows -----------------------------------------------------------------------------------------------------------------------------------
def test_windows_cut_rows_and_references_anywhere(ctx, monkeypatch):
    indexed, tokens, arrays = case_arrays("hamlet.is")
    words = read_classes(os.path.join(GOLD, "hamlet.colibri.cls"))
    want = b"".join(print_rows(words, arrays, tokens))
    for window in (None, 7, 1):
        if window:
            monkeypatch.setenv("COLIBRI_PRINT_WINDOW_BYTES", str(window))
        assert ctx.print_model(words, arrays, tokens) == want, window
        w, staging, scratch = ctx.print_info()
        B = min(window or (64 << 20), len(want))
        assert w == -(-len(want) // B) and staging == 2 * B and scratch > 0 and ctx.print_bytes == len(want)


# ---- random models -----------------------------------------------------------------------------------------------------------------------------
TIES = [(1234565, 10 ** 7), (1234575, 10 ** 7), (9999995, 10 ** 7), (99999950, 10 ** 12), (999999500, 10 ** 13), (5, 10 ** 6), (15, 10 ** 6), (1, 10 ** 7), (3, 4 * 10 ** 9)]


def random_print_model(rnd):
    """(words, arrays, tokens): n-grams, skipgrams with leading / trailing content and several gaps, flexgrams, multi-byte ids, ids without a
    word, empty words (the first one too), a redefined class 3, patterns without references, and counts / tokens that put the ties of
    test_print's formatter test into COVERAGE and FREQUENCY"""
    ids = [5, 6, 7, 8, 127, 128, 300, 20000, 2 ** 21 - 1, 2 ** 21 + 7]
    words = {3: rnd.choice([b"{*}", b"GAP"]), 4: b"{**}", 5: b"", 6: b"b", 7: b"cc", 127: b"edge", 128: b"two", 20000: b"three", 2 ** 21 - 1: "été".encode()}  # 8, 300, 2^21 + 7: no word
    keys = set()
    for _ in range(rnd.randint(0, 60)):
        n = rnd.randint(1, 6)
        toks = [rnd.choice(ids) for _ in range(n)]
        kind = rnd.random()
        if n >= 3 and kind < 0.35:
            for i in rnd.sample(range(1, n - 1), rnd.randint(1, n - 2)):
                toks[i] = 3
        elif n >= 3 and kind < 0.5:
            toks[rnd.randint(1, n - 2)] = 4
        keys.add(b"".join(varint(t) for t in toks))
    keys = sorted(keys, key=lambda k: rnd.random())
    tie = rnd.choice(TIES + [None])
    if tie:  # two unigrams in front: the first carries the tie, the second fills their group's total up
        keys = [varint(6), varint(7)] + [k for k in keys if k not in (varint(6), varint(7))]
    indexed = rnd.random() < 0.5
    tokens = rnd.randint(1, 5000)
    counts = [rnd.choice([0, 1, 2, 3, 7, 100, 65535, 2 ** 31 + 5]) for _ in keys]
    if tie:
        tokens = tie[1]  # COVERAGE of the first pattern = tie[0] / tie[1], and so is its FREQUENCY where the second count fits 32 bits
        counts = [tie[0], tie[1] - tie[0] if tie[1] - tie[0] < 2 ** 32 else 0] + [0] * (len(keys) - 2)
    key_off = np.cumsum([0] + [len(k) for k in keys]).astype(np.uint64)
    kb = np.frombuffer(b"".join(keys), dtype=np.uint8)
    if not indexed:
        return words, (key_off, kb, np.array(counts, dtype=np.uint32), None), tokens
    refs = [[(rnd.choice([1, 9, 10, 4294967295, rnd.randint(1, 10 ** 6)]), rnd.choice([0, 9, 10, 65535, rnd.randint(0, 999)])) for _ in range(rnd.choice([0, 1, 2, 5, 40]))] for _ in keys]
    ref_off = np.cumsum([0] + [len(r) for r in refs]).astype(np.uint64)
    rs = np.array([s for r in refs for s, _ in r], dtype=np.uint32)
    rt = np.array([t for r in refs for _, t in r], dtype=np.uint16)
    crafted = np.array(counts, dtype=np.uint32) if tie else None  # (crafted counts beside the references, or the references' own)
    return words, (key_off, kb, crafted, (ref_off, rs, rt)), tokens


def test_two_hundred_random_models(ctx, monkeypatch):
    rnd = random.Random(20260)
    checked, seen = 0, set()
    for i in range(200):
        words, arrays, tokens = random_print_model(rnd)
        if i % 2:
            monkeypatch.setenv("COLIBRI_PRINT_WINDOW_BYTES", str(rnd.randint(1, 9)))
        else:
            monkeypatch.delenv("COLIBRI_PRINT_WINDOW_BYTES", raising=False)
        want = b"".join(print_rows(words, arrays, tokens))
        assert ctx.print_model(words, arrays, tokens) == want, i
        for got, exp in zip(ctx.histogram(arrays), histogram_rows(arrays)):
            assert np.array_equal(got, exp), i
        seen |= {w for w in (b"skipgram", b"flexgram", b"{?}", b"inf", b"-nan", b"GAP", b"\t\n", b"0.0001\t", b"\t1\tngram", b"1e-07", b"0.123456\tngram\t1\t0.123456")
                 if w in want}
        seen.add("indexed" if arrays[3] is not None else "unindexed")
        checked += 1
    assert checked == 200 and len(seen) == 13, seen


# ---- balance -----------------------------------------------------------------------------------------------------------------------------------
def test_a_head_pattern_across_slices(ctx, monkeypatch):
    rnd = random.Random(5)
    digits = lambda d: rnd.randint(10 ** (d - 1), 10 ** d - 1)
    refs = {varint(6 + i): [(digits(rnd.randint(1, 9)), digits(rnd.randint(1, 4))) for _ in range(rnd.randint(0, 30))] for i in range(1, 51)}
    refs[varint(6)] = [(min(digits(1 + j % 10), 2 ** 32 - 1), min(digits(1 + j % 5), 65535)) for j in range(5000)]
    refs[varint(6)][-1] = (2 ** 32 - 1, 65535)
    key_off, kb, _, r = flat(refs)
    arrays = (key_off, kb, None, r)
    words = {6 + i: b"w%d" % i for i in range(60)}
    want = b"".join(print_rows(words, arrays, 123457))
    monkeypatch.setenv("COLIBRI_PRINT_SLICE", "64")
    monkeypatch.setenv("COLIBRI_PRINT_WINDOW_BYTES", "4096")
    assert ctx.print_model(words, arrays, 123457) == want
    assert ctx.print_info()[0] == -(-len(want) // 4096) > 10


# ---- a million tokens --------------------------------------------------------------------------------------------------------------------------
def test_device_against_host_at_a_million_tokens(ctx, tmp_path):
    from colibri_amd import synth
    vocab = 20_000
    payload = zipf_cached(1_000_000, vocab, 23)
    dat, clsf = tmp_path / "zipf.colibri.dat", tmp_path / "zipf.colibri.cls"
    dat.write_bytes(synth.HEADER + payload.tobytes())
    clsf.write_text("".join(f"{i}\tw{i}\n" for i in range(6, vocab - 50)))  # the highest ids have no word
    args = ["-f", str(dat), "-c", str(clsf), "-l", "4", "-t", "2", "-P"]
    digest = lambda out: hashlib.sha256(b"\n".join(sorted(out.split(b"\n")))).hexdigest()
    dev, err = cli(args, COLIBRI_PRINT="device")
    assert "(print on the device: uploaded model)" in err and dev.count(b"\n") > 100_000
    assert digest(dev) == digest(cli(args, COLIBRI_PRINT="host")[0])
    # the resident forms through the Python face: the same model where the training left it
    ctx.upload(bytes(payload))
    st = ctx.train(mintokens=2, maxlength=4, indexed=1)
    words = read_classes(str(clsf))
    res = ctx.print_model(words, None, st.totaltokens)
    assert digest(dev.split(b"\n", 1)[1]) == digest(res)
    key_off, key_bytes, counts, refs = ctx.export_arrays()
    arrays = (key_off, key_bytes[: int(key_off[-1])], None, refs)
    for cat, size in ((0, 0), (1, 2), (1, 4)):
        got = ctx.histogram(None, cat, size)
        exp = histogram_rows(arrays, cat, size) if cat else np.unique(counts, return_counts=True)
        assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1].astype(np.uint64)), (cat, size)
        up = ctx.histogram(arrays, cat, size)
        assert np.array_equal(got[0], up[0]) and np.array_equal(got[1], up[1])


# ---- refusals, fallbacks -----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(monkeypatch):
    from colibri_amd import capi
    indexed, tokens, arrays = case_arrays("hamlet.i")
    words = read_classes(os.path.join(GOLD, "hamlet.colibri.cls"))
    want = b"".join(print_rows(words, arrays, tokens))
    with capi.Context(0) as c:
        for call in (lambda: c.print_model(words, None, tokens), lambda: c.histogram(None)):  # an untrained context
            with pytest.raises(capi.ColibriError) as e:
                call()
            assert e.value.code == -6  # COLIBRI_ERR_STATE

        def stop(piece):
            raise RuntimeError("enough")
        monkeypatch.setenv("COLIBRI_PRINT_WINDOW_BYTES", "100")
        with pytest.raises(capi.ColibriError) as e:
            c.print_model(words, arrays, tokens, sink=stop)
        assert e.value.code == -6 and "sink" in str(e.value)
        assert c.print_model(words, arrays, tokens) == want
        monkeypatch.setenv("COLIBRI_PRINT_BUDGET", "1")
        with pytest.raises(capi.ColibriError) as e:
            c.print_model(words, arrays, tokens)
        assert e.value.code == -7 and "COLIBRI_PRINT_BUDGET" in str(e.value)  # COLIBRI_ERR_OVERFLOW
        monkeypatch.delenv("COLIBRI_PRINT_BUDGET")
        assert c.print_model(words, arrays, tokens) == want
        long_token = (np.array([0, 10], dtype=np.uint64), np.frombuffer(b"\x81" * 9 + b"\x01", dtype=np.uint8), np.array([1], dtype=np.uint32), None)
        with pytest.raises(capi.ColibriError) as e:
            c.print_model(words, long_token, tokens)
        assert e.value.code == -7 and "more than 9 bytes" in str(e.value)
        empty = (np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint32), None)
        assert c.print_model(words, empty, tokens) == b"" and c.print_info() == (0, 0, 0)
        assert [a.size for a in c.histogram(empty)] == [0, 0]
        assert c.print_model(words, arrays, tokens) == want


CALLER = r'''
#include <iostream>
#include "classdecoder.h"
#include "patternmodel.h"
int main(int argc, char** argv) {
    PatternModelOptions options;
    IndexedPatternModel<> model(argv[1], options);
    ClassDecoder decoder(argv[2]);
    if (argc > 3) std::cout << std::fixed;
    model.print(std::cout, decoder);
    return 0;
}
'''


def test_a_stream_out_of_its_default_state_prints_on_the_host(tmp_path):
    (tmp_path / "caller.cpp").write_text(CALLER)
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "colibri-core_amd", "host", "include"), "-I", os.path.join(ROOT, "include"), str(tmp_path / "caller.cpp"),
                           os.path.join(LIB, "libcolibri_amd_host.a"), "-L" + LIB, "-lcolibri_hip", "-Wl,-rpath," + LIB, "-L/opt/rocm/lib", "-lrccl", "-lamdhip64",
                           "-Wl,-rpath,/opt/rocm/lib", "-lpthread", "-o", str(tmp_path / "caller")])
    args = [str(tmp_path / "caller"), os.path.join(VIEWS, "hamlet.i.colibri.patternmodel"), os.path.join(GOLD, "hamlet.colibri.cls")]
    run = lambda a, mode: subprocess.run(a, capture_output=True, env={**os.environ, "COLIBRI_PRINT": mode}, timeout=300)
    dev, host = run(args, "device"), run(args, "host")
    assert dev.returncode == 0 and host.returncode == 0 and b"(print on the device: uploaded model)" in dev.stderr
    same_rows(dev.stdout, host.stdout)
    same_rows(dev.stdout, golden("hamlet.i", "print"))
    dev, host = run(args + ["fixed"], "device"), run(args + ["fixed"], "host")
    assert dev.returncode == 0 and b"default float state" in dev.stderr and b"on the device" not in dev.stderr
    assert dev.stdout == host.stdout and b"0.011299\t" in dev.stdout
