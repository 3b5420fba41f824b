"""Corpus decoding on the GPU (colibri-classdecode, ClassDecoder::decodefile, ctx.decode) against the reference's output
(tests/golden/decode/) and the restatement of tests/test_decode.py."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, zipf_cached
from test_decode import CASES, CLI, DEC, case_args, golden, read_classes, reference_decode

pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "colibri-core_amd", "bin")
LIB = os.path.join(ROOT, "colibri-core_amd", "lib")
IDS = [c["name"] for c in CASES]


@pytest.fixture(scope="module")
def ctx():
    from colibri_amd import capi
    with capi.Context(0) as c:
        yield c


def small_windows(monkeypatch, n="7"):
    monkeypatch.setenv("COLIBRI_DECODE_WINDOW_BYTES", n)


@pytest.mark.parametrize("window", [None, "5"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_cli_matches_the_reference(case, window):
    env = dict(os.environ)
    if window:
        env["COLIBRI_DECODE_WINDOW_BYTES"] = window
    r = subprocess.run([CLI, "-c", os.path.join(GOLDEN, case["classes"]), "-f", os.path.join(GOLDEN, case["data"])] + case["options"], capture_output=True, env=env,
                       timeout=300)
    want_out, want_err = golden(case)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert r.stdout == want_out
    assert r.stderr.decode() == want_err


CALLER = r'''
#include <iostream>
#include <sstream>
#include <cstdlib>
#include "classdecoder.h"
// argv: class file, data file, start, end, mode (0: decodefile to cout, 1: decodefiletostring, 2: getdataversion + decodefile_v1)
int main(int argc, char** argv) {
    ClassDecoder d(argv[1]);
    const unsigned s = std::atoi(argv[3]), e = std::atoi(argv[4]);
    const int mode = std::atoi(argv[5]);
    if (mode == 0) d.decodefile(argv[2], std::cout, s, e);
    if (mode == 1) std::cout << d.decodefiletostring(argv[2], s, e);
    if (mode == 2) {
        std::ifstream in(argv[2], std::ios::binary);
        if (getdataversion(in) != 1) return 5;
        d.decodefile_v1(in, std::cout, s, e, true);
    }
    return 0;
}
'''


@pytest.fixture(scope="module")
def caller(tmp_path_factory):
    d = tmp_path_factory.mktemp("decode_caller")
    (d / "caller.cpp").write_text(CALLER)
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "colibri-core_amd", "host", "include"), "-I", os.path.join(ROOT, "include"), str(d / "caller.cpp"),
                           os.path.join(LIB, "libcolibri_amd_host.a"), "-L" + LIB, "-lcolibri_hip", "-Wl,-rpath," + LIB, "-L/opt/rocm/lib", "-lrccl", "-lamdhip64",
                           "-Wl,-rpath,/opt/rocm/lib", "-lpthread", "-o", str(d / "caller")])
    return str(d / "caller")


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_cxx_face_decodefile_and_decodefiletostring(caller, case):
    s, e = case_args(case)
    args = [caller, os.path.join(GOLDEN, case["classes"]), os.path.join(GOLDEN, case["data"]), str(s), str(e)]
    want_out, want_err = golden(case)
    r = subprocess.run(args + ["0"], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert r.stdout == want_out and r.stderr.decode() == want_err
    r = subprocess.run(args + ["1"], capture_output=True, timeout=300)  # (quiet by default, as in the reference)
    assert r.returncode == 0 and r.stdout == want_out and r.stderr == b""
    if case["data"].endswith("v1.colibri.dat"):
        r = subprocess.run(args + ["2"], capture_output=True, timeout=300)
        assert r.returncode == 0 and r.stdout == want_out


def payload_of(data):
    """(version, payload without header) as the C ABI takes them"""
    if data[:1] == b"\xa2":
        return (1 if data[1:2] == b"\x01" else 2), data[2:]
    return 1, data


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_ctx_decode_matches_the_reference(ctx, case, monkeypatch):
    cls = read_classes(open(os.path.join(GOLDEN, case["classes"]), "rb").read())
    version, payload = payload_of(open(os.path.join(GOLDEN, case["data"]), "rb").read())
    s, e = case_args(case)
    want_out, want_err = golden(case)
    assert ctx.decode(cls, payload, version, s, e) == want_out
    assert f"Processed {ctx.decode_lines} lines\n" == want_err
    small_windows(monkeypatch, "3")
    assert ctx.decode(cls, payload, version, s, e) == want_out
    if want_out:
        assert ctx.decode_info()[0] == (len(want_out) + 2) // 3


def random_v1(rng, nlines, vocab):
    out = bytearray()
    for _ in range(nlines):
        for _ in range(int(rng.integers(0, 9))):
            r = rng.random()
            if r < 0.12:
                out.append(128 if r < 0.06 else 129)
            elif r < 0.14:
                out.append(int(rng.integers(130, 256)))  # ignored
            else:
                v = int(rng.choice([0, 1, 2, 3, 4, 5, int(rng.integers(6, 6 + vocab)), 300, 70000, 16777216]))
                b = v.to_bytes(max(1, (v.bit_length() + 7) // 8), "little")
                out += bytes([len(b)]) + b
        out.append(0)
    if rng.random() < 0.3:
        out = out[:-1]  # no final 00
    return bytes(out)


def random_classes(rng, ids):
    cls = {1: b"{|}", 2: b"{?}", 3: b"{*}", 4: b"{**}"}
    for k in ids:
        if rng.random() < 0.8:
            cls[int(k)] = bytes(rng.integers(33, 127, size=int(rng.integers(0, 12))).astype(np.uint8)) + (b"\r" if rng.random() < 0.05 else b"")
    if rng.random() < 0.3:
        cls[3] = b"SKIP"
    if rng.random() < 0.2:
        cls[0] = b"zero"
    return cls


def random_range(rng, nlines):
    kind = rng.integers(0, 4)
    if kind == 0:
        return 0, 0
    a, b = (int(x) for x in rng.integers(0, nlines + 3, size=2))
    return (a, b) if kind != 3 else (max(a, b) + 2, min(a, b))


def test_random_corpora_against_the_restatement(ctx, monkeypatch):
    from colibri_amd import synth
    rng = np.random.default_rng(20261016)
    checked = 0
    for it in range(200):
        v1 = it % 4 == 3
        if v1:
            nlines = int(rng.integers(1, 60))
            data = random_v1(rng, nlines, 40)
            payload, version, whole = data, 1, b"\xa2\x01" + data  # (the restatement reads a whole file: A2 01 = v1 data after the header)
            cls = random_classes(rng, list(range(5, 46)) + [300, 70000])
        else:
            nlines = int(rng.integers(1, 80))
            payload = synth.random_corpus(rng, nsent=nlines, maxlen=int(rng.integers(1, 14)), vocab=int(rng.integers(2, 40)), big_classes=bool(rng.random() < 0.7),
                                          empty_rate=float(rng.random() * 0.3))
            if rng.random() < 0.2:
                payload = payload[:-1]  # no final 00
            if rng.random() < 0.1:
                payload += b"\x85\x81"  # a truncated varint
            version, whole = 2, synth.HEADER + payload
            cls = random_classes(rng, list(range(1, 50)) + [127, 128, 129, 16383, 16384, 2097152])
        s, e = random_range(rng, nlines)
        want, err = reference_decode(cls, whole, s, e)
        monkeypatch.delenv("COLIBRI_DECODE_WINDOW_BYTES", raising=False)
        assert ctx.decode(cls, payload, version, s, e) == want, (it, s, e)
        assert f"Processed {ctx.decode_lines} lines\n" == err
        small_windows(monkeypatch, str(int(rng.integers(1, 9))))
        assert ctx.decode(cls, payload, version, s, e) == want, (it, s, e, "small windows")
        checked += 1
    assert checked == 200


def numpy_decode(payload, words, start=0, end=0):
    """the restatement for a v2 payload of canonical varints ending in 00, in numpy: words = {id: bytes}"""
    b = np.frombuffer(payload, dtype=np.uint8)
    term = b < 128
    tid = np.concatenate([[0], np.cumsum(term)[:-1]])  # token of every byte
    tstart = np.flatnonzero(np.concatenate([[True], term[:-1]]))
    k = np.arange(b.size) - tstart[tid]
    ids = np.bincount(tid, weights=(b & 127).astype(np.float64) * (128.0 ** k)).astype(np.int64)
    delim = ids == 0
    line = np.concatenate([[1], 1 + np.cumsum(delim)[:-1]])
    show = (start == 0 and end == 0) | (line >= start) | (line <= end)
    first = np.concatenate([[True], delim[:-1]])
    top = max(words)
    table = np.empty(top + 1, dtype=object)
    table[:] = b""
    for w, t in words.items():
        table[w] = t
    pieces = np.where(delim, b"\n", np.where(first, b"", b" ") + table[np.minimum(ids, top)] * (ids <= top))
    return b"".join(pieces[show].tolist())


def zipf_words(vocab):
    return {i: f"w{i}".encode() for i in range(6, vocab + 6)} | {1: b"{|}", 2: b"{?}", 3: b"{*}", 4: b"{**}"}


def test_ten_million_tokens_against_numpy(ctx):
    payload = bytes(zipf_cached(10_000_000, 50_000, 91))
    words = zipf_words(50_000 - 100)  # the highest ids have no word
    for s, e in ((0, 0), (200_000, 100_000), (3, 0)):
        got = ctx.decode(words, payload, 2, s, e)
        assert hashlib.sha256(got).hexdigest() == hashlib.sha256(numpy_decode(payload, words, s, e)).hexdigest(), (s, e)
    w, staging, scratch = ctx.decode_info()
    assert w >= 1 and staging >= 2 and scratch > 0


def test_round_trip_at_a_hundred_million_tokens(tmp_path):
    """decode a 10^8-token corpus with the CLI, re-encode the text with colibri-classencode -c and its own class file: the same bytes"""
    from colibri_amd import synth
    vocab = 100_000
    payload = zipf_cached(100_000_000, vocab, 17)
    dat = tmp_path / "zipf.colibri.dat"
    dat.write_bytes(synth.HEADER + payload.tobytes())
    clsf = tmp_path / "zipf.colibri.cls"
    clsf.write_text("".join(f"{i}\tw{i}\n" for i in range(6, vocab + 6)))
    txt = tmp_path / "round.txt"
    with open(txt, "wb") as f:
        r = subprocess.run([CLI, "-c", str(clsf), "-f", str(dat)], stdout=f, stderr=subprocess.PIPE, timeout=900)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    r = subprocess.run([os.path.join(BIN, "colibri-classencode"), "-c", str(clsf), "-o", "out", str(txt)], cwd=tmp_path, capture_output=True, timeout=900)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    digest = lambda p: hashlib.sha256(open(p, "rb").read()).hexdigest()
    assert digest(tmp_path / "round.colibri.dat") == digest(dat)


def test_the_largest_id_of_the_table_bound(ctx):
    from colibri_amd import capi, synth
    top = capi.DECODE_MAX_IDS - 1
    payload = synth.encode_v2(np.array([6, top, 0, top, 6, 0], dtype=np.uint32)).tobytes()
    assert ctx.decode({6: b"a", top: b"TOP"}, payload) == b"a TOP\nTOP a\n"
    assert ctx.decode({6: b"a"}, payload) == b"a \n a\n"  # (the class map ends below: a small table)
    big = synth.encode_v2(np.array([6, top + 1, 0], dtype=np.uint32)).tobytes()
    assert ctx.decode({6: b"a"}, big) == b"a \n"
    with pytest.raises(capi.ColibriError, match="bound"):
        ctx.decode({6: b"a", top + 1: b"X"}, big)
    assert ctx.decode({6: b"a"}, payload, 2, 2, 0) == b" a\n"  # the context is usable after the refusal (line 1 hidden)


def test_refusals(ctx):
    from colibri_amd import capi
    import ctypes as C
    huge = np.zeros(0xFFFFFF00, dtype=np.uint8)  # (calloc'd: untouched pages; the size is refused before any byte is read)
    for version in (2, 1):
        mc = C.c_uint64()
        rc = ctx.L.colibri_decode_upload(ctx.h, huge.ctypes.data, huge.size, version, C.byref(mc))
        assert rc == -5 and "4 GiB per-device limit" in ctx.L.colibri_last_error(ctx.h).decode()
    del huge
    with pytest.raises(capi.ColibriError, match="more than 5 bytes"):
        ctx.decode({6: b"a"}, b"\x86\x80\x80\x80\x80\x01\x00")
    with pytest.raises(capi.ColibriError, match="id 0"):
        ctx.decode({6: b"a"}, b"\x06\x80\x00\x00")
    assert ctx.decode({6: b"a", 0: b"z"}, b"\x02\x00\x00\x01\x06\x00", 1) == b"z a\n"  # (in v1, id 0 is a word)
    assert ctx.decode({6: b"a"}, b"") == b"" and ctx.decode_lines == 0


def test_empty_data_file(tmp_path):
    """no specification exists for a zero-byte file (the reference reads an uninitialised byte): empty output, "Processed 0 lines" """
    empty = tmp_path / "empty.colibri.dat"
    empty.write_bytes(b"")
    r = subprocess.run([CLI, "-c", os.path.join(GOLDEN, "hamlet.colibri.cls"), "-f", str(empty)], capture_output=True, timeout=120)
    assert r.returncode == 0 and r.stdout == b"" and r.stderr == b"Processed 0 lines\n"
