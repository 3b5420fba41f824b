#!/usr/bin/env python3
"""Measurements for DESIGN.md §5j: the C++ face's train() with -p 4 through the host route and through the device route of the same build.

  python tools/subsume_probe.py [--tokens 1000000 10000000] [--vocab 100000] [--maxlength 5] [--prune 4] [--repeat 3]

The corpus is bench.py's (synth.zipf_corpus, seed 7) at each of --tokens. Two kinds of figure, one JSON line each:
  "device call"  colibri_subsume_resident + colibri_subsume_fetch on the model resident after train(), unindexed and indexed: wall time of the
                 calls (they end in a device synchronise), patterns before and after, levels, look-ups, scratch peak
  "cli"          colibri-patternmodeller -f <corpus> -t 2 -l <maxlength> [-u] -p <prune> (no output model, no view: train() alone) under
                 COLIBRI_SUBSUME=host and =device, alternating: wall time of the whole process, and the prune step alone as train() reports it
                 under COLIBRI_HOST_TIMING (on the host route it contains the node map the route walks)
Every timing: one untimed warm-up, then --repeat timed runs; the median and all values are printed. Take them on an otherwise idle device."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "colibri-core_amd", "pyhost"))
CLI = os.path.join(ROOT, "colibri-core_amd", "bin", "colibri-patternmodeller")
STEP = re.compile(r"COLIBRI_HOST_TIMING subsume ([0-9.e+-]+) ms on the (\w+), (\d+) patterns left")


def device_calls(args, tokens, payload):
    from colibri_amd import capi
    with capi.Context(0) as ctx:
        ctx.upload(payload)
        for indexed in (0, 1):
            st = ctx.train(mintokens=2, maxlength=args.maxlength, indexed=indexed)
            ms = []
            for r in range(args.repeat + 1):
                t0 = time.perf_counter()
                ctx.subsume(prunenonsubsumed=args.prune, maxlength=args.maxlength, resident=True)
                if r:
                    ms.append((time.perf_counter() - t0) * 1e3)
            levels, probes, scratch = ctx.subsume_info()
            print(json.dumps({"what": "device call", "tokens": tokens, "indexed": indexed, "patterns": int(st.npatterns), "kept": ctx.subsume_kept, "levels": levels, "probes": probes,
                              "scratch_bytes": scratch, "ms_median": statistics.median(ms), "ms": ms}), flush=True)


def cli(args, tokens, payload):
    from colibri_amd import synth
    with tempfile.TemporaryDirectory() as d:
        dat = os.path.join(d, "probe.colibri.dat")
        with open(dat, "wb") as f:
            f.write(synth.HEADER + payload)
        for indexed in (0, 1):
            wall, step, left = {"host": [], "device": []}, {"host": [], "device": []}, {}
            for r in range(args.repeat + 1):  # (run 0 of each route is the warm-up; the routes alternate)
                for route in ("host", "device"):
                    t0 = time.perf_counter()
                    p = subprocess.run([CLI, "-f", dat, "-t", "2", "-l", str(args.maxlength), "-p", str(args.prune)] + ([] if indexed else ["-u"]), stdout=subprocess.DEVNULL,
                                       stderr=subprocess.PIPE, text=True, env={**os.environ, "COLIBRI_SUBSUME": route, "COLIBRI_HOST_TIMING": "1"})
                    w = (time.perf_counter() - t0) * 1e3
                    assert p.returncode == 0, p.stderr[-2000:]
                    m = STEP.search(p.stderr)
                    assert m and m.group(2) == route, p.stderr[-2000:]
                    left[route] = int(m.group(3))
                    if r:
                        wall[route].append(w)
                        step[route].append(float(m.group(1)))
            assert left["host"] == left["device"]
            print(json.dumps({"what": "cli", "tokens": tokens, "indexed": indexed, "patterns_left": left["host"],
                              "host_step_ms_median": statistics.median(step["host"]), "device_step_ms_median": statistics.median(step["device"]),
                              "host_wall_ms_median": statistics.median(wall["host"]), "device_wall_ms_median": statistics.median(wall["device"]),
                              "host_step_ms": step["host"], "device_step_ms": step["device"], "host_wall_ms": wall["host"], "device_wall_ms": wall["device"]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--vocab", type=int, default=100_000)
    ap.add_argument("--maxlength", type=int, default=5)
    ap.add_argument("--prune", type=int, default=4)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--no-cli", action="store_true")
    args = ap.parse_args()
    from colibri_amd import synth
    for tokens in args.tokens:
        payload = bytes(synth.zipf_corpus(tokens, args.vocab, 7, header=False))
        device_calls(args, tokens, payload)
        if not args.no_cli:
            cli(args, tokens, payload)


if __name__ == "__main__":
    main()
