"""Corpus decoding (colibri-classdecode; reference src/classdecode.cpp, ClassDecoder in src/classdecoder.cpp).

CPU part: a restatement of the reference's specification (`reference_decode` below), checked against the real reference's stdout and stderr
on every fixture case (tests/golden/decode/, see the README there); the CLI's refusals that need no device; the host-only ClassDecoder
methods (decodeseq, add, prune) through a small caller. The GPU part (tests/test_gpu_decode.py) holds the device, the C++ face and the CLI
against the fixtures and this restatement."""
import gzip
import json
import os
import subprocess

import pytest

from conftest import GOLDEN, ROOT

DEC = os.path.join(GOLDEN, "decode")
CLI = os.path.join(ROOT, "colibri-core_amd", "bin", "colibri-classdecode")
CASES = json.load(open(os.path.join(DEC, "cases.json")))
PRESET = {2: b"{?}", 3: b"{*}", 4: b"{**}", 1: b"{|}"}  # classdecoder.cpp:91-94


def c_atoi(text):
    """atoi() of the bytes before the first tab: leading white space, a sign, digits; strtol's clamp, then int, then unsigned int"""
    s = text.lstrip(b" \t\n\v\f\r")
    sign = 1
    if s[:1] in (b"+", b"-"):
        sign = -1 if s[:1] == b"-" else 1
        s = s[1:]
    digits = b""
    for ch in s:
        if 48 <= ch <= 57:
            digits += bytes([ch])
        else:
            break
    v = sign * int(digits or b"0")
    v = max(-(1 << 63), min((1 << 63) - 1, v))
    return v & 0xFFFFFFFF


def read_classes(data):
    """ClassDecoder::load (classdecoder.cpp:84-126): presets for 1-4, then one line at a time, id = atoi of the text before the first tab,
    word = everything after it (later tabs and a \\r stay); a later line overrides an earlier one; lines without a tab are skipped"""
    cls = dict(PRESET)
    for line in data.split(b"\n"):
        t = line.find(b"\t")
        if t >= 0:
            cls[c_atoi(line[:t])] = line[t + 1:]
    return cls


def shown(line, start, end):
    """classdecoder.cpp:181, :191, :211, :218"""
    return (start == 0 and end == 0) or line >= start or line <= end


def reference_decode(cls, data, start=0, end=0):
    """ClassDecoder::decodefile / decodefile_v1 (classdecoder.cpp:166-238) as colibri-classdecode prints them -> (stdout, stderr).
    cls: {id: word bytes}; data: the whole .colibri.dat. A token whose id has no word prints as the empty string (the map's operator[]).
    Where the reference has no defined behaviour: an empty file (an uninitialised byte) prints nothing; a v1 token cut off by the end of the
    file is dropped; a v1 id is its first four base-256 digits, unsigned (the reference's int overflows beyond 2^31)."""
    out = []
    lines = 0
    if len(data) == 0:
        return b"", "Processed 0 lines\n"
    if data[0] == 0xA2:  # getdataversion (:259-284): A2 <version>; any version other than 1 takes the v2 path
        version = data[1] if len(data) > 1 else 0
        body = data[2:]
    elif data[0] > 5:
        raise ValueError("plain text")
    else:
        version, body = 1, data
    line, first = 1, True
    if version != 1:
        i, n = 0, len(body)
        while i < n:
            v, k = 0, 0
            while i < n and body[i] >= 128:  # little-endian base 128, high bit on all bytes but the last
                v |= (body[i] & 127) << (7 * k)
                i += 1
                k += 1
            if i >= n:
                break  # a trailing varint cut off: dropped (:49-51, :179-180)
            v |= body[i] << (7 * k)
            i += 1
            if v == 0:
                if shown(line, start, end):
                    out.append(b"\n")
                first = True
                line += 1
            elif shown(line, start, end):
                if not first:
                    out.append(b" ")
                out.append(cls.get(v, b""))
                first = False
    else:
        i, n = 0, len(body)
        while i < n:
            c = body[i]
            i += 1
            if c == 0:
                if shown(line, start, end):
                    out.append(b"\n")
                line += 1
                first = True
            elif c < 128:
                if i + c > n:
                    break
                digits = body[i:i + c]
                i += c
                if shown(line, start, end):
                    v = int.from_bytes(digits[:4], "little")
                    if not first:
                        out.append(b" ")
                    out.append(cls.get(v, b""))
                    first = False
            elif c in (128, 129):  # printed whatever line it is in (:222-233)
                if not first:
                    out.append(b" ")
                out.append(b"{*}" if c == 128 else b"{**}")
                first = False
    lines = line - 1
    return b"".join(out), f"Processed {lines} lines\n"


def case_args(case):
    s = e = 0
    o = case["options"]
    for j in range(0, len(o), 2):
        if o[j] == "-s":
            s = int(o[j + 1])
        elif o[j] == "-e":
            e = int(o[j + 1])
    return s, e


def golden(case):
    with gzip.open(os.path.join(DEC, case["stdout"]), "rb") as f:
        return f.read(), case["stderr"]


def case_inputs(case):
    cls = read_classes(open(os.path.join(GOLDEN, case["classes"]), "rb").read())
    data = open(os.path.join(GOLDEN, case["data"]), "rb").read()
    return cls, data


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_restatement_matches_the_reference(case):
    cls, data = case_inputs(case)
    s, e = case_args(case)
    out, err = reference_decode(cls, data, s, e)
    want_out, want_err = golden(case)
    assert len(want_out) == case["stdout_bytes"]
    assert out == want_out
    assert err == want_err


def test_fixtures_cover_the_issue():
    names = {c["name"] for c in CASES}
    for corpus in ("hamlet.v2", "hamlet.v1", "phrases15k", "zipf"):
        assert {corpus, corpus + "_s5", corpus + "_e4", corpus + "_s3e10", corpus + "_s9e2"} <= names
    assert {"apology", "edge", "markers_s4e1"} <= names
    apology = next(c for c in CASES if c["name"] == "apology")
    assert golden(apology)[0] == open(os.path.join(GOLDEN, "classenc", "apology.txt"), "rb").read()  # decoding undoes the encoder


def run(args, **kw):
    if not os.path.exists(CLI):
        pytest.fail(f"{CLI} is not built (python -c 'import __graft_entry__ as g; g.build()')")
    return subprocess.run([CLI] + args, capture_output=True, timeout=120, **kw)


def test_cli_without_arguments_prints_usage_and_exits_2():
    r = run([])
    assert r.returncode == 2
    assert b"Syntax: colibri-classdecode" in r.stderr and r.stdout == b""
    assert run(["-c", os.path.join(GOLDEN, "hamlet.colibri.cls")]).returncode == 2
    assert run(["-f", os.path.join(GOLDEN, "hamlet.v2.colibri.dat")]).returncode == 2


def test_cli_missing_class_file_exits_3(tmp_path):
    missing = str(tmp_path / "none.colibri.cls")
    r = run(["-c", missing, "-f", os.path.join(GOLDEN, "hamlet.v2.colibri.dat")])
    assert r.returncode == 3
    assert r.stderr.decode().splitlines()[-1] == f"File does not exist: {missing}"


def test_cli_refuses_an_unknown_option():
    r = run(["-x", "-c", os.path.join(GOLDEN, "hamlet.colibri.cls"), "-f", os.path.join(GOLDEN, "hamlet.v2.colibri.dat")])
    assert r.returncode == 2  # (the reference abort()s)
    assert b"Unknown option: -x" in r.stderr


def test_cli_unreadable_or_plain_text_data_file(tmp_path):
    cls = os.path.join(GOLDEN, "hamlet.colibri.cls")
    r = run(["-c", cls, "-f", str(tmp_path / "none.colibri.dat")])
    assert r.returncode not in (0, -6, 134)
    assert b"ERROR: Supplied data file can not be opened. Check whether it exists and whether you have proper permissions..." in r.stderr
    r = run(["-c", cls, "-f", os.path.join(GOLDEN, "classenc", "apology.txt")])
    assert r.returncode not in (0, -6, 134)
    assert b"ERROR: Supplied data file is not a valid Colibri Data file, did you pass plain-text instead perhaps?..." in r.stderr
    assert r.stdout == b""


CALLER = r'''
#include <iostream>
#include "classdecoder.h"
int main(int argc, char** argv) {
    ClassDecoder d(argv[1]);
    for (const std::string& w : d.decodeseq({6, 7, 99999, 3})) std::cout << "[" << w << "]";
    std::cout << " " << d.size() << " " << d.hasclass(99999) << "\n";
    d.add(70000, "added");
    std::cout << d.gethighestclass() << " " << d[70000] << "\n";
    d.prune(8);
    std::cout << d.gethighestclass() << " " << d.hasclass(7) << d.hasclass(8) << d.hasclass(70000) << d.hasclass(3) << "\n";
    return 0;
}
'''


def test_host_only_methods_of_classdecoder(tmp_path):
    """decodeseq (an id without a word gives "" and enters the map, classdecoder.cpp:132-138), add, prune (:240-257): host code"""
    lib = os.path.join(ROOT, "colibri-core_amd", "lib")
    src = tmp_path / "caller.cpp"
    src.write_text(CALLER)
    exe = tmp_path / "caller"
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "colibri-core_amd", "host", "include"), "-I", os.path.join(ROOT, "include"), str(src),
                           os.path.join(lib, "libcolibri_amd_host.a"), "-L" + lib, "-lcolibri_hip", "-Wl,-rpath," + lib, "-L/opt/rocm/lib", "-lrccl", "-lamdhip64",
                           "-Wl,-rpath,/opt/rocm/lib", "-lpthread", "-o", str(exe)])
    cls = os.path.join(DEC, "crafted.colibri.cls")
    out = subprocess.run([str(exe), cls], capture_output=True, text=True, timeout=60, check=True).stdout.splitlines()
    n = len(read_classes(open(cls, "rb").read()))
    assert out[0] == f"[SIX-again][seven\twith tab][][SKIP-override] {n + 1} 1"
    assert out[1] == "3000000 added"  # (the crafted class file already holds 3000000)
    assert out[2] == "7 1001"
