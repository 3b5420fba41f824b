#!/usr/bin/env python3
"""Measurements for DESIGN.md §5m: the skipgrams of the indexed model a colibri_train left in HBM (colibri_modelskip_resident) beside what the
same skipgrams cost inside a training run of the same build on the same device.

  python tools/modelskip_probe.py [--tokens 100000000] [--vocab 1000000] [--maxlength 5] [--skiptypes 2] [--repeat 10]

The corpus is bench.py's (synth.zipf_corpus, seed 7). One JSON line each:
  "in-train"   train_ms of colibri_train indexed alone and indexed with skipgrams, alternating; the yardstick is the difference of the medians
  "modelskip"  after an indexed colibri_train without skipgrams: colibri_modelskip_resident (no fetch), wall time around the call (it ends in a
               device synchronise) and, from a profiled train's context, the kernel time of its classes (colibri_kernel_time: `skipgram` =
               validity, candidates, grouping, verdicts, keys; `index` = the surviving groups' references gathered and sorted; `export` = the
               resident model's key bytes gathered for the view); the per-order figures, candidates and scratch peak of the call
Every timing: one untimed warm-up, then --repeat timed runs; the median, the extremes and all values are printed. Take them on an otherwise idle device."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "colibri-core_amd", "pyhost"))


def spread(ms):
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "all": ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=100_000_000)
    ap.add_argument("--vocab", type=int, default=1_000_000)
    ap.add_argument("--maxlength", type=int, default=5)
    ap.add_argument("--skiptypes", type=int, default=2)
    ap.add_argument("--repeat", type=int, default=10)
    args = ap.parse_args()
    from colibri_amd import capi, synth
    payload = synth.zipf_corpus(args.tokens, args.vocab, 7, header=False)
    opts = dict(mintokens=2, minskiptypes=args.skiptypes, maxlength=args.maxlength)
    with capi.Context(0) as ctx:
        ctx.upload(payload)
        plain, skip = [], []
        for r in range(args.repeat + 1):  # (run 0 of each is the warm-up; the two alternate)
            a = ctx.train(mintokens=2, maxlength=args.maxlength, indexed=1).train_ms
            st = ctx.train(mintokens=2, maxlength=args.maxlength, indexed=1, doskipgrams=1, minskiptypes=args.skiptypes)
            if r:
                plain.append(a)
                skip.append(st.train_ms)
        print(json.dumps({"what": "in-train", "tokens": args.tokens, "patterns_with_skipgrams": int(st.npatterns), "indexed_ms": spread(plain), "indexed_skipgrams_ms": spread(skip),
                          "yardstick_ms": statistics.median(skip) - statistics.median(plain)}), flush=True)
        st = ctx.train(mintokens=2, maxlength=args.maxlength, indexed=1, profile=1)  # (the context keeps bracketing kernel classes with events afterwards)
        wall, k_skip, k_index, k_export = [], [], [], []
        for r in range(args.repeat + 1):
            s0, i0, e0 = ctx.kernel_time(capi.K_SKIPGRAM)[0], ctx.kernel_time(capi.K_INDEX)[0], ctx.kernel_time(capi.K_EXPORT)[0]
            t0 = time.perf_counter()
            n, kb, nr, gone = ctx.model_skipgrams_sizes(resident=True, **opts)
            w = (time.perf_counter() - t0) * 1e3
            if r:
                wall.append(w)
                k_skip.append(ctx.kernel_time(capi.K_SKIPGRAM)[0] - s0)
                k_index.append(ctx.kernel_time(capi.K_INDEX)[0] - i0)
                k_export.append(ctx.kernel_time(capi.K_EXPORT)[0] - e0)
        orders, candidates, scratch = ctx.model_skipgrams_info()
        print(json.dumps({"what": "modelskip", "tokens": args.tokens, "patterns": int(st.npatterns), "references": int(st.nrefs), "skipgrams": n, "key_bytes": kb, "skipgram_references": nr,
                          "erased": gone, "orders": orders, "candidates": candidates, "scratch_bytes": scratch, "wall_ms": spread(wall), "kernel_skipgram_ms": spread(k_skip),
                          "kernel_index_ms": spread(k_index), "kernel_export_ms": spread(k_export)}), flush=True)
        plain_wall = []
        st = ctx.train(mintokens=2, maxlength=args.maxlength, indexed=1)  # (and without the event brackets)
        for r in range(args.repeat + 1):
            t0 = time.perf_counter()
            ctx.model_skipgrams_sizes(resident=True, **opts)
            if r:
                plain_wall.append((time.perf_counter() - t0) * 1e3)
        print(json.dumps({"what": "modelskip unprofiled", "tokens": args.tokens, "wall_ms": spread(plain_wall)}), flush=True)


if __name__ == "__main__":
    main()
