"""Throughput of the pattern relations (colibri-patternmodeller --subsumes / --subsumed / --leftneighbours / --rightneighbours) on one MI355X.
The model is the indexed n-gram model of a Zipf corpus (synth.zipf_corpus), trained on the device and left resident;
colibri_relations_resident then runs each of the four kinds on it. Reported per kind: wall time of the call (it ends with a device
synchronisation; the rows stay on the device), related occurrences (events), chunks, peak scratch HBM, rows. Prints one JSON object per line;
numbers go into DESIGN.md."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "colibri-core_amd", "pyhost"))

KINDS = (("subchildren", 0), ("subparents", 1), ("leftneighbours", 2), ("rightneighbours", 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=10_000_000)
    ap.add_argument("--vocab", type=int, default=100_000)
    ap.add_argument("--maxlength", type=int, default=3)
    ap.add_argument("--mintokens", type=int, default=2)
    ap.add_argument("--threshold", type=int, default=0)
    ap.add_argument("--reps", type=int, default=2)
    a = ap.parse_args()
    from colibri_amd import capi, synth
    payload = synth.zipf_corpus(a.tokens, a.vocab, 61, header=False)
    with capi.Context(0) as ctx:
        ctx.upload(payload)
        st = ctx.train(mintokens=a.mintokens, maxlength=a.maxlength, indexed=1)
        npat, _, nrefs = ctx.result_sizes()
        for name, kind in KINDS:
            best, rows = None, 0
            for _ in range(a.reps):
                n = capi.C.c_uint64()
                t0 = time.perf_counter()
                rc = ctx.L.colibri_relations_resident(ctx.h, kind, a.threshold, capi.C.byref(n))
                ms = (time.perf_counter() - t0) * 1e3
                ctx._check(rc)
                best, rows = (ms if best is None else min(best, ms)), n.value
            events, chunks, scratch = ctx.relations_info()
            print(json.dumps({"kind": name, "tokens": a.tokens, "vocab": a.vocab, "maxlength": a.maxlength, "mintokens": a.mintokens, "threshold": a.threshold,
                              "patterns": npat, "references": nrefs, "train_ms": round(st.train_ms, 3), "relations_ms": round(best, 3), "events": events,
                              "events_per_s": round(events / (best / 1e3)), "chunks": chunks, "scratch_bytes": scratch, "rows": rows}), flush=True)


if __name__ == "__main__":
    main()
