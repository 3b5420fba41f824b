#!/usr/bin/env python3
"""Measurements for DESIGN.md §5k: the skipgrams of an in-place rebuild (-I -s) through the host route and through the device route of the same build.

  python tools/recount_probe.py [--tokens 1000000 10000000] [--vocab 100000] [--maxlength 4] [--threshold 10] [--repeat 3]

The corpus is synth.zipf_corpus (seed 7, with phrases, so that skipgrams turn up) at each of --tokens. A model is trained on it once with -s; then,
one JSON line each:
  "device call"  colibri_recount + colibri_recount_fetch of the model's skipgrams on the uploaded corpus, unindexed and indexed: wall time of the
                 calls (they end in a device synchronise), skipgrams, (length, mask) groups, occurrences, chunks, scratch peak
  "cli"          colibri-patternmodeller -I -i <model> -f <corpus> -s -t <threshold> [-u] (no output model, no view) under COLIBRI_RECOUNT=host and
                 =device, alternating: wall time of the whole process, and the skipgram step alone as train() reports it under COLIBRI_HOST_TIMING
The parent of this feature refused the run, so the host route is the yardstick. Every timing: one untimed warm-up, then --repeat timed runs; the
median and all values are printed. Take them on an otherwise idle device."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "colibri-core_amd", "pyhost"))
CLI = os.path.join(ROOT, "colibri-core_amd", "bin", "colibri-patternmodeller")
STEP = re.compile(r"COLIBRI_HOST_TIMING recount ([0-9.e+-]+) ms on the (\w+), (\d+) skipgrams, (\d+) occurrences")
INFO = re.compile(r"COLIBRI_HOST_TIMING recount groups (\d+) chunks (\d+) scratch (\d+) bytes references (\d+)")


def skipgram_keys(ctx):
    """the skipgrams of the model the context just trained, in export layout"""
    key_off, key_bytes, _, _ = ctx.export_arrays()
    kb, off = key_bytes.tobytes(), [int(x) for x in key_off]
    keys = []
    for j in range(len(off) - 1):
        k, start = kb[off[j]:off[j + 1]], 0
        for i, b in enumerate(k):
            if b < 128:
                if i == start and b == 3:
                    keys.append(k)
                    break
                start = i + 1
    return np.cumsum([0] + [len(k) for k in keys]).astype(np.uint64), np.frombuffer(b"".join(keys) + b"\0", dtype=np.uint8)[:-1], len(keys)


def device_calls(args, tokens, payload):
    from colibri_amd import capi
    with capi.Context(0) as ctx:
        ctx.upload(payload)
        ctx.train(mintokens=args.threshold, maxlength=args.maxlength, indexed=1, doskipgrams=1)
        ko, kb, nkeys = skipgram_keys(ctx)
        for indexed in (0, 1):
            ms = []
            for r in range(args.repeat + 1):
                t0 = time.perf_counter()
                counts, _, rs, _ = ctx.recount(ko, kb, indexed=indexed, mintokens=args.threshold)
                if r:
                    ms.append((time.perf_counter() - t0) * 1e3)
            groups, chunks, scratch = ctx.recount_info()
            print(json.dumps({"what": "device call", "tokens": tokens, "indexed": indexed, "skipgrams": nkeys, "kept": ctx.recount_kept, "groups": groups,
                              "occurrences": int(counts.astype(np.uint64).sum()), "references": len(rs), "chunks": chunks, "scratch_bytes": scratch,
                              "ms_median": statistics.median(ms), "ms": ms}), flush=True)


def cli(args, tokens, payload):
    from colibri_amd import synth
    with tempfile.TemporaryDirectory() as d:
        dat, model = os.path.join(d, "probe.colibri.dat"), os.path.join(d, "probe.colibri.patternmodel")
        with open(dat, "wb") as f:
            f.write(synth.HEADER + payload)
        subprocess.run([CLI, "-f", dat, "-t", str(args.threshold), "-l", str(args.maxlength), "-s", "-o", model], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, check=True)
        for indexed in (0, 1):
            wall, step, seen, info = {"host": [], "device": []}, {"host": [], "device": []}, {}, None
            for r in range(args.repeat + 1):  # (run 0 of each route is the warm-up; the routes alternate)
                for route in ("host", "device"):
                    t0 = time.perf_counter()
                    p = subprocess.run([CLI, "-I", "-i", model, "-f", dat, "-s", "-t", str(args.threshold), "-l", str(args.maxlength)] + ([] if indexed else ["-u"]),
                                       stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, env={**os.environ, "COLIBRI_RECOUNT": route, "COLIBRI_HOST_TIMING": "1"})
                    w = (time.perf_counter() - t0) * 1e3
                    assert p.returncode == 0, p.stderr[-2000:]
                    m = STEP.search(p.stderr)
                    assert m and m.group(2) == route, p.stderr[-2000:]
                    seen[route] = (int(m.group(3)), int(m.group(4)))
                    if route == "device":
                        info = INFO.search(p.stderr)
                    if r:
                        wall[route].append(w)
                        step[route].append(float(m.group(1)))
            assert seen["host"] == seen["device"], seen
            print(json.dumps({"what": "cli", "tokens": tokens, "indexed": indexed, "skipgrams": seen["host"][0], "occurrences": seen["host"][1],
                              "chunks": int(info.group(2)) if info else None, "scratch_bytes": int(info.group(3)) if info else None,
                              "host_step_ms_median": statistics.median(step["host"]), "device_step_ms_median": statistics.median(step["device"]),
                              "host_wall_ms_median": statistics.median(wall["host"]), "device_wall_ms_median": statistics.median(wall["device"]),
                              "host_step_ms": step["host"], "device_step_ms": step["device"], "host_wall_ms": wall["host"], "device_wall_ms": wall["device"]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--vocab", type=int, default=100_000)
    ap.add_argument("--maxlength", type=int, default=4)
    ap.add_argument("--threshold", type=int, default=10)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--no-cli", action="store_true")
    args = ap.parse_args()
    from colibri_amd import synth
    for tokens in args.tokens:
        payload = bytes(synth.zipf_corpus(tokens, args.vocab, 7, phrases=True, header=False))
        device_calls(args, tokens, payload)
        if not args.no_cli:
            cli(args, tokens, payload)


if __name__ == "__main__":
    main()
