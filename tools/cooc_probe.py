"""Throughput of sentence co-occurrence (colibri-patternmodeller -C / -Y) on one MI355X. The model is the indexed n-gram model of a Zipf corpus
(synth.zipf_corpus), trained on the device and left resident; colibri_cooc_resident then runs -C <threshold> and -Y <x> on it. Reported per
mode: wall time of the call (it ends with a device synchronisation; the rows stay on the device), pair events, chunks, peak scratch HBM, rows.
Prints one JSON object per line; numbers go into DESIGN.md."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "colibri-core_amd", "pyhost"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=10_000_000)
    ap.add_argument("--vocab", type=int, default=100_000)
    ap.add_argument("--maxlength", type=int, default=3)
    ap.add_argument("--mintokens", type=int, default=2)
    ap.add_argument("--threshold", type=int, default=2)
    ap.add_argument("--npmi", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=2)
    a = ap.parse_args()
    from colibri_amd import capi, synth
    payload = synth.zipf_corpus(a.tokens, a.vocab, 61, header=False)
    with capi.Context(0) as ctx:
        ctx.upload(payload)
        st = ctx.train(mintokens=a.mintokens, maxlength=a.maxlength, indexed=1)
        npat, _, nrefs = ctx.result_sizes()
        for mode, name in ((capi.COOC_COUNT, "C"), (capi.COOC_NPMI, "Y")):
            best = None
            for _ in range(a.reps):
                t0 = time.perf_counter()
                n = ctx.L.colibri_cooc_resident(ctx.h, a.threshold if mode == capi.COOC_COUNT else 0, mode, a.npmi, capi.C.byref(capi.C.c_uint64()))
                ms = (time.perf_counter() - t0) * 1e3
                ctx._check(n)
                best = ms if best is None else min(best, ms)
            events, chunks, scratch = ctx.cooc_info()
            a_, b_, c_, v_ = ctx.cooc_resident(a.threshold if mode == capi.COOC_COUNT else 0, mode, a.npmi)
            print(json.dumps({"mode": "-" + name, "tokens": a.tokens, "vocab": a.vocab, "maxlength": a.maxlength, "mintokens": a.mintokens,
                              "threshold": a.threshold if mode == capi.COOC_COUNT else a.npmi, "patterns": npat, "references": nrefs,
                              "train_ms": round(st.train_ms, 3), "cooc_ms": round(best, 3), "pair_events": events, "events_per_s": round(events / (best / 1e3)),
                              "chunks": chunks, "scratch_bytes": scratch, "rows": int(len(a_))}), flush=True)


if __name__ == "__main__":
    main()
