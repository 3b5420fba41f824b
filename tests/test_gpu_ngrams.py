"""N-gram extraction on the GPU (colibri-extractngrams, colibri_host::extract_ngrams, ctx.ngrams) against the reference's output
(tests/golden/ngrams/) and the restatement of tests/test_ngrams.py.

Output windows (COLIBRI_NGRAMS_WINDOW_BYTES): 1, 3, 5, 7 put the windows' edges inside words, on spaces and on newlines, 16 and 17 on both sides of a
16-byte piece. Every golden case runs at the default window and at each of the six through all three faces, one test per (case, window). A window
costs two launches, a copy and an event wait, 12 to 18 us, so the time of a pair is its number of windows: through ctx.ngrams the whole matrix
runs (its longest pair, apology.t3U_n40 at 1 byte, is 740 k windows and took 12.9 s); through the two faces that start a process per run the two pairs of
more than PROCESS_MAX_WINDOWS windows are left out by name (PROCESS_EXCLUDED): the library cuts the windows below all three faces."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from test_ngrams import CASES, CLI, case_inputs, golden, reference_ngrams, want_of

pytestmark = pytest.mark.gpu
LIB = os.path.join(ROOT, "colibri-core_amd", "lib")
WINDOWS = [1, 3, 5, 7, 16, 17]
PROCESS_MAX_WINDOWS = 250_000  # some 4 s of windows beside the process' start
# the (case, window) pairs the CLI and the C++ face do not run, with their windows and what they took through ctx.ngrams on an MI355X; ctx.ngrams runs them
PROCESS_EXCLUDED = {
    ("apology_n4", 1): "391 367 windows, 4.6 s",
    ("apology.t3U_n40", 1): "739 878 windows, 12.9 s",
}
PAIRS = [(c, w) for c in CASES for w in [None] + WINDOWS]
PAIR_IDS = [f"{c['name']}-w{w or 'default'}" for c, w in PAIRS]
PROCESS_PAIRS = [(c, w) for c, w in PAIRS if (c["name"], w) not in PROCESS_EXCLUDED]
PROCESS_IDS = [f"{c['name']}-w{w or 'default'}" for c, w in PROCESS_PAIRS]
K_BLOCK = 256  # kernels.hpp: threads per block; a scan tile is 4 * K_BLOCK inputs


@pytest.fixture(scope="module")
def ctx():
    from colibri_amd import capi
    with capi.Context(0) as c:
        yield c


def ceil_div(a, b):
    return (a + b - 1) // b


def test_the_excluded_pairs_are_the_ones_above_the_bound():
    above = {(c["name"], w) for c in CASES for w in WINDOWS if ceil_div(c["stdout_bytes"], w) > PROCESS_MAX_WINDOWS}
    assert above == set(PROCESS_EXCLUDED)


@pytest.mark.parametrize("case,window", PAIRS, ids=PAIR_IDS)
def test_ctx_ngrams_matches_the_reference(ctx, case, window, monkeypatch):
    cls, data = case_inputs(case)
    want = want_of(case)
    if window:
        monkeypatch.setenv("COLIBRI_NGRAMS_WINDOW_BYTES", str(window))
    else:
        monkeypatch.delenv("COLIBRI_NGRAMS_WINDOW_BYTES", raising=False)
    assert ctx.ngrams(cls, data[2:], case["n"]) == want
    assert ctx.ngrams_count == want.count(b"\n") and ctx.ngrams_bytes == len(want)
    windows, staging, scratch = ctx.ngrams_info()
    assert windows == (ceil_div(len(want), window) if window else (1 if want else 0))
    if want:
        assert staging == 2 * min(window or len(want), len(want)) and scratch > 0


def run_tool(args, window=None):
    env = dict(os.environ)
    env.pop("COLIBRI_NGRAMS_WINDOW_BYTES", None)
    if window:
        env["COLIBRI_NGRAMS_WINDOW_BYTES"] = str(window)
    return subprocess.run(args, capture_output=True, env=env, timeout=300)


def tool_args(case):
    return ["-c", os.path.join(GOLDEN, case["classes"]), "-n", str(case["n"]), os.path.join(GOLDEN, case["data"])]


@pytest.mark.parametrize("case,window", PROCESS_PAIRS, ids=PROCESS_IDS)
def test_cli_matches_the_reference(case, window):
    r = run_tool([CLI] + tool_args(case), window)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert r.stdout == want_of(case) and r.stderr == b""


def test_cli_several_data_files_and_the_default_n():
    hamlet = next(c for c in CASES if c["name"] == "hamlet.v2_n3")
    dat = os.path.join(GOLDEN, hamlet["data"])
    r = run_tool([CLI, "-c", os.path.join(GOLDEN, hamlet["classes"]), dat, dat])  # (-n absent: 3)
    assert r.returncode == 0 and r.stdout == golden(hamlet) * 2 and r.stderr == b""


CALLER = r'''
#include <iostream>
#include <cstdlib>
#include "classdecoder.h"
// argv: class file, data file, n
int main(int argc, char** argv) {
    if (argc < 4) return 9;
    const ClassDecoder d(argv[1]);
    const uint64_t rows = colibri_host::extract_ngrams(d, argv[2], std::atoi(argv[3]), std::cout);
    std::cout.flush();
    std::cerr << rows;
    return 0;
}
'''


@pytest.fixture(scope="module")
def caller(tmp_path_factory):
    d = tmp_path_factory.mktemp("ngrams_caller")
    (d / "caller.cpp").write_text(CALLER)
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "colibri-core_amd", "host", "include"), "-I", os.path.join(ROOT, "include"), str(d / "caller.cpp"),
                           os.path.join(LIB, "libcolibri_amd_host.a"), "-L" + LIB, "-lcolibri_hip", "-Wl,-rpath," + LIB, "-L/opt/rocm/lib", "-lrccl", "-lamdhip64",
                           "-Wl,-rpath,/opt/rocm/lib", "-lpthread", "-o", str(d / "caller")])
    return str(d / "caller")


def caller_args(caller, case):
    return [caller, os.path.join(GOLDEN, case["classes"]), os.path.join(GOLDEN, case["data"]), str(case["n"])]


@pytest.mark.parametrize("case,window", PROCESS_PAIRS, ids=PROCESS_IDS)
def test_cxx_face_matches_the_reference(caller, case, window):
    r = run_tool(caller_args(caller, case), window)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    want = want_of(case)
    assert r.stdout == want and r.stderr == str(want.count(b"\n")).encode()


# ---- random corpora against the restatement ----------------------------------------------------------------------------------------------------
def random_corpus(rng, nlines):
    """lines of 0-9 tokens with runs of empty lines, ids up to 2^21 (1- to 4-byte varints), a fifth of them without a word, some empty words"""
    from colibri_amd import synth
    pool = np.unique(np.concatenate([np.arange(1, 40), rng.integers(40, 1 << 14, 40), rng.integers(1 << 14, (1 << 21) + 1, 40), [127, 128, 16383, 16384, 1 << 21]]))
    cls = {}
    for k in pool:
        r = rng.random()
        if r < 0.2:
            continue  # no word: {?}
        cls[int(k)] = b"" if r < 0.3 else bytes(rng.integers(33, 127, size=int(rng.integers(1, 12))).astype(np.uint8))
    syms = []
    while nlines > 0:
        if rng.random() < 0.15:
            run = int(rng.integers(1, 6))  # a run of empty lines
            syms += [0] * run
            nlines -= run
            continue
        syms += [int(x) for x in rng.choice(pool, size=int(rng.integers(0, 10)))] + [0]
        nlines -= 1
    if rng.random() < 0.4 and len(syms) > 1:
        syms.pop()  # no final 00
    return cls, synth.encode_v2(np.array(syms, dtype=np.uint32)).tobytes()


def test_random_corpora_against_the_restatement(ctx, monkeypatch):
    rng = np.random.default_rng(20261021)
    checked = 0
    for it in range(24):
        cls, payload = random_corpus(rng, int(rng.integers(1, 400)))
        for n in range(1, 11):
            want = reference_ngrams(cls, b"\xa2\x02" + payload, n)
            monkeypatch.delenv("COLIBRI_NGRAMS_WINDOW_BYTES", raising=False)
            got = ctx.ngrams(cls, payload, n) if n == 1 else ctx.ngrams_again(n)
            assert got == want, (it, n)
            assert ctx.ngrams_count == want.count(b"\n") and ctx.ngrams_bytes == len(want)
            w = int(rng.choice([1, 2, 3, 15, 16, 17, 31, 33, 4095, 4096, 4097]))
            if ceil_div(len(want), w) <= 5000:
                monkeypatch.setenv("COLIBRI_NGRAMS_WINDOW_BYTES", str(w))
                assert ctx.ngrams_again(n) == want, (it, n, w)
                assert ctx.ngrams_info()[0] == ceil_div(len(want), w)
            checked += 1
    assert checked == 24 * 10


def exact_positions(rng, npos):
    """a corpus of exactly npos positions (tokens and 00s): lines of 1-7 tokens of the ids 6 .. 29"""
    from colibri_amd import synth
    syms = []
    while len(syms) < npos:
        syms += [int(x) for x in rng.integers(6, 30, size=int(rng.integers(1, 8)))] + [0]
    syms = syms[:npos]
    return synth.encode_v2(np.array(syms, dtype=np.uint32)).tobytes(), syms


@pytest.mark.parametrize("npos", [K_BLOCK - 1, K_BLOCK, K_BLOCK + 1, 4 * K_BLOCK - 1, 4 * K_BLOCK, 4 * K_BLOCK + 1, 9 * K_BLOCK + 5])
def test_block_and_scan_tile_edges(ctx, npos, monkeypatch):
    """the positions, and with them the n-grams of n = 1, cross a block (K_BLOCK) and a scan tile (4 * K_BLOCK); words of one byte, empty words (every
    n-gram of n = 1 is its newline alone) and longer ones"""
    rng = np.random.default_rng(npos)
    payload, syms = exact_positions(rng, npos)
    assert len(payload) == npos
    for words in ({k: bytes([59 + k]) for k in range(6, 30)}, {k: b"" for k in range(6, 30)}, {k: (b"w%d" % k) * (k - 5) for k in range(6, 28)}):
        for n in (1, 2, 7):
            want = reference_ngrams(words, b"\xa2\x02" + payload, n)
            monkeypatch.delenv("COLIBRI_NGRAMS_WINDOW_BYTES", raising=False)
            assert ctx.ngrams(words, payload, n) == want, n
            monkeypatch.setenv("COLIBRI_NGRAMS_WINDOW_BYTES", str(K_BLOCK + 1))  # every window starts in another lane's n-gram
            assert ctx.ngrams_again(n) == want, n


def test_one_byte_ngrams_and_runs_of_empty_lines(ctx, monkeypatch):
    """50 000 one-token lines of an empty word, n = 1: the text is 50 000 newlines; and n-grams with three 00s between them"""
    monkeypatch.delenv("COLIBRI_NGRAMS_WINDOW_BYTES", raising=False)
    assert ctx.ngrams({6: b""}, b"\x06\x00" * 50_000, 1) == b"\n" * 50_000
    assert ctx.ngrams_count == 50_000
    assert ctx.ngrams({7: b"x"}, b"\x06\x00\x00\x00" * 20_000, 1) == b"{?}\n" * 20_000  # runs of empty lines between the n-grams: no entries, no bytes


# ---- more than 2^32 bytes of text from a small upload ------------------------------------------------------------------------------------------
def test_output_beyond_4_gib(ctx, monkeypatch):
    from colibri_amd import capi
    monkeypatch.delenv("COLIBRI_NGRAMS_WINDOW_BYTES", raising=False)
    word = bytes(np.random.default_rng(4096).integers(33, 127, size=4096).astype(np.uint8))
    row = np.frombuffer(word + b"\n", dtype=np.uint8)
    lines = 1_100_000
    total = lines * row.size
    assert total > (1 << 32) + (64 << 20)
    payload = np.frombuffer(b"\x06\x00" * lines, dtype=np.uint8)
    mc = C.c_uint64()
    ctx._check(ctx.L.colibri_decode_upload(ctx.h, payload.ctypes.data, payload.size, 2, C.byref(mc)))
    ctx._print_classes({6: word})
    B = 64 << 20
    seen = {"bytes": 0, "calls": 0, "kept": {}}

    def take(_user, p, nbytes):  # keeps the byte count, and the windows either side of offset 2^32
        start = seen["bytes"]
        if start < (1 << 32) + B and start + nbytes > (1 << 32) - B:
            seen["kept"][start] = np.ctypeslib.as_array(p, shape=(nbytes,)).copy()
        seen["bytes"] += nbytes
        seen["calls"] += 1
        return 0
    nb, ng = C.c_uint64(), C.c_uint64()
    ctx._check(ctx.L.colibri_ngrams(ctx.h, 1, capi.DecodeSink(take), None, C.byref(nb), C.byref(ng)))
    assert nb.value == total == seen["bytes"] and ng.value == lines
    assert ctx.ngrams_info()[0] == seen["calls"] == ceil_div(total, B)
    assert sorted(seen["kept"]) == [(1 << 32) - B, 1 << 32]  # (2^32 is a window edge at the default window)
    for start, got in seen["kept"].items():
        first = start % row.size
        assert np.array_equal(got, np.tile(row, ceil_div(first + got.size, row.size))[first:first + got.size]), start


def test_words_and_rows_of_4_mib(ctx, monkeypatch):
    """the scans add the 1024 lengths of a tile in 32 bits, so a word or a row of 4 MiB or more is refused; one byte less prints"""
    from colibri_amd import capi
    monkeypatch.delenv("COLIBRI_NGRAMS_WINDOW_BYTES", raising=False)
    limit = 1 << 22
    word = b"x" * (limit - 2)
    assert ctx.ngrams({6: word}, b"\x06\x00", 1) == word + b"\n"  # a row of limit - 1 bytes
    with pytest.raises(capi.ColibriError, match="4 MiB") as e:
        ctx.ngrams({6: word + b"x"}, b"\x06\x00", 1)  # a row of limit bytes
    assert e.value.code == -7
    half = b"y" * (limit // 2)
    with pytest.raises(capi.ColibriError, match="4 MiB"):
        ctx.ngrams({6: half}, b"\x06\x06\x00", 2)  # two words below the limit, their row above
    assert ctx.ngrams({6: half}, b"\x06\x06\x00", 1) == (half + b"\n") * 2  # usable afterwards
    with pytest.raises(capi.ColibriError, match="4 MiB"):
        ctx.ngrams({6: word + b"xx", 7: b"z"}, b"\x06\x00\x07\x07\x00", 2)  # a word at the limit in a line too short for an n-gram


# ---- states and refusals -----------------------------------------------------------------------------------------------------------------------
def test_states_and_refusals(monkeypatch):
    from colibri_amd import capi
    monkeypatch.delenv("COLIBRI_NGRAMS_WINDOW_BYTES", raising=False)
    words = {6: b"a", 7: b"b"}
    payload = b"\x06\x07\x06\x00\x07\x00"
    with capi.Context(0) as c:
        with pytest.raises(capi.ColibriError, match="no corpus uploaded by colibri_decode_upload") as e:
            c.ngrams_again(1)
        assert e.value.code == -6
        buf = np.frombuffer(payload, dtype=np.uint8)
        c._check(c.L.colibri_decode_upload(c.h, buf.ctypes.data, buf.size, 2, None))
        with pytest.raises(capi.ColibriError, match="no word table installed by colibri_print_classes") as e:
            c.ngrams_again(1)
        assert e.value.code == -6
        assert c.ngrams(words, payload, 2) == b"a b\nb a\n" and c.ngrams_count == 2  # usable after both
        with pytest.raises(capi.ColibriError, match="n must be at least 1") as e:
            c.ngrams_again(0)
        assert e.value.code == -1
        assert c.L.colibri_ngrams(c.h, 1, capi.DecodeSink(), None, None, None) == -1  # (a null sink)
        assert c.ngrams_again(1) == b"a\nb\na\nb\n"
        # an upload made with version 1
        v1 = np.frombuffer(b"\x01\x06\x01\x07\x00", dtype=np.uint8)
        c._check(c.L.colibri_decode_upload(c.h, v1.ctypes.data, v1.size, 1, None))
        with pytest.raises(capi.ColibriError, match="version 1") as e:
            c.ngrams_again(1)
        assert e.value.code == -4
        assert c.ngrams(words, payload, 3) == b"a b a\n"
        # n above the longest line: nothing, no windows
        assert c.ngrams_again(4) == b"" and c.ngrams_count == 0 and c.ngrams_bytes == 0
        assert c.ngrams_info()[0] == 0 and c.ngrams_info()[1] == 0
        assert c.ngrams_again(0xFFFFFFFF) == b"" and c.ngrams_count == 0  # (i + n does not wrap)
        assert c.ngrams(words, b"", 1) == b"" and c.ngrams_info()[0] == 0
        # a sink that stops after the first window
        monkeypatch.setenv("COLIBRI_NGRAMS_WINDOW_BYTES", "3")
        pieces = []

        def stop(piece):
            pieces.append(bytes(piece))
            raise RuntimeError("enough")
        with pytest.raises(capi.ColibriError, match="the sink stopped the call") as e:
            c.ngrams(words, payload, 1, sink=stop)
        assert e.value.code == -6 and pieces == [b"a\nb"] and c.ngrams_count == 0
        assert c.ngrams_again(1) == b"a\nb\na\nb\n" and c.ngrams_info()[0] == 3
        # tokens the decoder refuses are refused with its messages
        with pytest.raises(capi.ColibriError, match="more than 5 bytes"):
            c.ngrams(words, b"\x86\x80\x80\x80\x80\x01\x00", 1)
        with pytest.raises(capi.ColibriError, match="id 0"):
            c.ngrams(words, b"\x06\x80\x00\x00", 1)
        assert c.ngrams(words, payload + b"\x85\x81", 2) == b"a b\nb a\n"  # a last varint cut off by the end of the data is dropped (§5d)
