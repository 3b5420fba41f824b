#!/usr/bin/env python3
"""Measurements for DESIGN.md §5f: colibri_print_model_resident into a discarding sink (wall time of the call, bytes, windows, scratch peak),
indexed and unindexed, and the CLI's -P under COLIBRI_PRINT=device against host (wall time, peak resident set of the children so far).

  python tools/print_probe.py --tokens 10000000 [--vocab 100000] [--maxlength 5] [--cli] [--repeat 3]

One JSON line per measurement. Timings are of single calls after one untimed warm-up call; take them on an otherwise idle device."""
import argparse
import json
import os
import resource
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "colibri-core_amd", "pyhost"))
CLI = os.path.join(ROOT, "colibri-core_amd", "bin", "colibri-patternmodeller")


def words_for(vocab):
    return {i: f"w{i}".encode() for i in range(6, vocab + 6)} | {1: b"{|}", 2: b"{?}", 3: b"{*}", 4: b"{**}"}


def resident(args, payload):
    from colibri_amd import capi
    words = words_for(args.vocab)
    with capi.Context(0) as ctx:
        ctx.upload(payload)
        for indexed in (1, 0):
            st = ctx.train(mintokens=2, maxlength=args.maxlength, indexed=indexed)
            discard = lambda piece: None
            ctx.print_model(words, None, st.totaltokens, sink=discard)  # warm-up: allocations, the pinned staging
            times = []
            for _ in range(args.repeat):
                t0 = time.perf_counter()
                ctx.print_model(words, None, st.totaltokens, sink=discard)
                times.append((time.perf_counter() - t0) * 1e3)
            w, staging, scratch = ctx.print_info()
            t0 = time.perf_counter()
            counts, patterns = ctx.histogram(None)
            hist_ms = (time.perf_counter() - t0) * 1e3
            print(json.dumps({"what": "print_model_resident", "tokens": args.tokens, "indexed": indexed, "train_ms": st.train_ms, "print_ms": times, "outbytes": ctx.print_bytes,
                              "windows": w, "staging_bytes": staging, "scratch_bytes": scratch, "histogram_ms": hist_ms, "histogram_rows": int(counts.size)}), flush=True)


def cli(args, payload):
    from colibri_amd import synth
    with tempfile.TemporaryDirectory() as d:
        dat, cls = os.path.join(d, "probe.colibri.dat"), os.path.join(d, "probe.colibri.cls")
        with open(dat, "wb") as f:
            f.write(synth.HEADER + payload)
        with open(cls, "w") as f:
            f.write("".join(f"{i}\tw{i}\n" for i in range(6, args.vocab + 6)))
        for mode in ("device", "host"):  # (ru_maxrss is the largest child so far: the second figure is an upper bound for its own run only if it is the larger)
            t0 = time.perf_counter()
            with open(os.devnull, "wb") as null:
                p = subprocess.run([CLI, "-f", dat, "-c", cls, "-l", str(args.maxlength), "-t", "2", "-P"], stdout=null, stderr=subprocess.PIPE, env={**os.environ, "COLIBRI_PRINT": mode})
            wall = time.perf_counter() - t0
            print(json.dumps({"what": "cli -P", "tokens": args.tokens, "mode": mode, "wall_s": wall, "returncode": p.returncode,
                              "children_maxrss_kb": resource.getrusage(resource.RUSAGE_CHILDREN).ru_maxrss}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=10_000_000)
    ap.add_argument("--vocab", type=int, default=100_000)
    ap.add_argument("--maxlength", type=int, default=5)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--cli", action="store_true")
    args = ap.parse_args()
    from colibri_amd import synth
    payload = bytes(synth.zipf_corpus(args.tokens, args.vocab, 7, header=False))
    resident(args, payload)
    if args.cli:
        cli(args, payload)


if __name__ == "__main__":
    main()
