#!/usr/bin/env python3
"""Measurements for DESIGN.md §5i: a model queried with N of its own sentences, through the host route and through the device route of the same
build.

  python tools/query_probe.py [--tokens 10000000] [--vocab 100000] [--maxlength 5] [--lines 100000] [--repeat 5]

The corpus is bench.py's (synth.zipf_corpus, seed 7) at --tokens. Two kinds of figure, one JSON line each:
  "device calls"  colibri_query_resident + colibri_query_fetch, and colibri_query_text into a discarding sink, on the model resident after
                  train(): wall time of the calls (they end in a device synchronise), rows, bytes, chunks, windows, scratch peak
  "cli"           colibri-patternmodeller -i <model> -c <cls> --queryfile <lines> under COLIBRI_QUERY=host and =device, alternating: wall time of the
                  whole process (loading the model included), output bytes
Every timing: one untimed warm-up, then --repeat timed runs; the median and all values are printed. Take them on an otherwise idle device."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "colibri-core_amd", "pyhost"))
CLI = os.path.join(ROOT, "colibri-core_amd", "bin", "colibri-patternmodeller")


def words_for(vocab):
    return {i: f"w{i}".encode() for i in range(6, vocab + 6)} | {1: b"{|}", 2: b"{?}", 3: b"{*}", 4: b"{**}"}


def first_lines(payload, n):
    """the first n sentences of a class-encoded corpus (every 00 closes one), as one payload"""
    end, pos = 0, -1
    for _ in range(n):
        pos = payload.find(b"\x00", pos + 1)
        if pos < 0:
            break
        end = pos + 1
    return payload[:end]


def timed(fn, repeat):
    fn()
    out = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def device_calls(args, payload, lines):
    from colibri_amd import capi
    words = words_for(args.vocab)
    with capi.Context(0) as ctx:
        ctx.upload(payload)
        for indexed in (0, 1):
            st = ctx.train(mintokens=2, maxlength=args.maxlength, indexed=indexed)
            got = {}

            def rows():
                got["rows"] = len(ctx.query(lines, resident=True, minlength=1, maxlength=args.maxlength)[1])
            q_ms = timed(rows, args.repeat)
            # (the text of the resident indexed model is not timed: its rows carry all their references, so every occurrence of a frequent
            # pattern repeats that pattern's whole reference list — terabytes at this size; the CLI's rows have no references)
            t_ms = timed(lambda: ctx.query_text(words, st.totaltokens, sink=lambda piece: None), args.repeat) if not indexed else []
            if indexed:
                ctx.query_bytes = 0
            chunks, windows, staging, scratch = ctx.query_info()
            print(json.dumps({"what": "device calls", "tokens": args.tokens, "indexed": indexed, "patterns": int(st.npatterns), "lines": args.lines, "query_bytes": len(lines),
                              "rows": got["rows"], "query_ms_median": statistics.median(q_ms), "query_ms": q_ms, "text_ms_median": statistics.median(t_ms) if t_ms else None, "text_ms": t_ms,
                              "text_bytes": ctx.query_bytes, "chunks": chunks, "windows": windows, "staging_bytes": staging, "scratch_bytes": scratch}), flush=True)


def cli(args, payload, lines):
    from colibri_amd import synth
    with tempfile.TemporaryDirectory() as d:
        dat, cls, model, qf = (os.path.join(d, n) for n in ("probe.colibri.dat", "probe.colibri.cls", "probe.colibri.patternmodel", "lines.txt"))
        with open(dat, "wb") as f:
            f.write(synth.HEADER + payload)
        with open(cls, "w") as f:
            f.write("".join(f"{i}\tw{i}\n" for i in range(6, args.vocab + 6)))
        subprocess.run([CLI, "-f", dat, "-l", str(args.maxlength), "-t", "2", "-u", "-o", model], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        text = []
        for sent in lines.split(b"\x00")[:-1]:  # the lines as text: the words of their tokens
            ids, cur, shift = [], 0, 0
            for b in sent:
                cur |= (b & 127) << shift
                shift += 7
                if b < 128:
                    ids.append(cur)
                    cur, shift = 0, 0
            text.append(" ".join(f"w{i}" for i in ids))
        with open(qf, "w") as f:
            f.write("\n".join(text) + "\n")
        times, nbytes = {"host": [], "device": []}, {}
        for r in range(args.repeat + 1):  # (run 0 of each mode is the warm-up; the modes alternate)
            for mode in ("host", "device"):
                t0 = time.perf_counter()
                p = subprocess.run([CLI, "-i", model, "-u", "-c", cls, "--queryfile", qf], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, env={**os.environ, "COLIBRI_QUERY": mode})
                wall = (time.perf_counter() - t0) * 1e3
                assert p.returncode == 0, mode
                nbytes[mode] = len(p.stdout)
                if r:
                    times[mode].append(wall)
        assert nbytes["host"] == nbytes["device"]
        print(json.dumps({"what": "cli", "tokens": args.tokens, "lines": args.lines, "output_bytes": nbytes["host"], "host_ms_median": statistics.median(times["host"]),
                          "host_ms": times["host"], "device_ms_median": statistics.median(times["device"]), "device_ms": times["device"]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=10_000_000)
    ap.add_argument("--vocab", type=int, default=100_000)
    ap.add_argument("--maxlength", type=int, default=5)
    ap.add_argument("--lines", type=int, default=100_000)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--no-cli", action="store_true")
    args = ap.parse_args()
    from colibri_amd import synth
    payload = bytes(synth.zipf_corpus(args.tokens, args.vocab, 7, header=False))
    lines = first_lines(payload, args.lines)
    device_calls(args, payload, lines)
    if not args.no_cli:
        cli(args, payload, lines)


if __name__ == "__main__":
    main()
