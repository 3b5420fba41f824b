"""Cost of the coverage report (colibri-patternmodeller -R; colibri_coverage, csrc/coverage.hpp) on one MI355X.
The model is the indexed n-gram model of a Zipf corpus (synth.zipf_corpus, the one bench.py builds), trained on the device and left resident.
Reported: colibri_coverage_resident and colibri_coverage (the exported model uploaded again), best of --reps wall times of the call (each ends
with a device synchronisation), with the mark kernel's test-before-set on and off (COLIBRI_COV_TEST), references marked, bitmap bytes, peak scratch.
With --cli the corpus is also written to a file and `colibri-patternmodeller -f corpus -R` and `-i model -R` are timed end to end under
COLIBRI_REPORT=host and =device (wall time, peak resident set of the child). Prints one JSON object per line; numbers go into DESIGN.md §5e."""
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


def best_of(reps, call):
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = call()
        ms = (time.perf_counter() - t0) * 1e3
        best = ms if best is None else min(best, ms)
    return best, out


def timed_cli(args, mode):
    before = resource.getrusage(resource.RUSAGE_CHILDREN).ru_maxrss
    t0 = time.perf_counter()
    p = subprocess.run([CLI] + args, capture_output=True, env={**os.environ, "COLIBRI_REPORT": mode})
    s = time.perf_counter() - t0
    rss = resource.getrusage(resource.RUSAGE_CHILDREN).ru_maxrss  # (the largest child so far: run the lighter mode first)
    return {"cli": " ".join(a for a in args if a.startswith("-")), "mode": mode, "returncode": p.returncode, "wall_s": round(s, 3),
            "peak_rss_mb_children": round(max(before, rss) / 1024, 1), "covered_row": next((ln for ln in p.stdout.decode().splitlines() if ln.startswith("Covered:")), "")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=100_000_000)
    ap.add_argument("--vocab", type=int, default=100_000)
    ap.add_argument("--maxlength", type=int, default=5)
    ap.add_argument("--mintokens", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cli", action="store_true", help="also time the CLI end to end under COLIBRI_REPORT=host / device")
    a = ap.parse_args()
    from colibri_amd import capi, synth
    payload = synth.zipf_corpus(a.tokens, a.vocab, 61, header=False)
    base = {"tokens": a.tokens, "vocab": a.vocab, "maxlength": a.maxlength, "mintokens": a.mintokens}
    with capi.Context(0) as ctx:
        ctx.upload(payload)
        st = ctx.train(mintokens=a.mintokens, maxlength=a.maxlength, indexed=1)
        npat, _, nrefs = ctx.result_sizes()
        base.update({"patterns": npat, "references": nrefs, "train_ms": round(st.train_ms, 3)})
        key_off, key_bytes, counts, (ref_off, rs, rt) = ctx.export_arrays()
        for test in ("1", "0"):
            os.environ["COLIBRI_COV_TEST"] = test
            for per_size in (False, True):
                ms, got = best_of(a.reps, lambda: ctx.coverage_resident(per_size=per_size))
                marked, bitmap, scratch = ctx.coverage_info()
                print(json.dumps({**base, "form": "resident", "test_before_set": test == "1", "per_size": per_size, "coverage_ms": round(ms, 3), "references_marked": marked,
                                  "bitmap_bytes": bitmap, "scratch_bytes": scratch, "covered_tokens": int(got[3][0][0]), "types": int(got[2][0][0])}), flush=True)
        os.environ["COLIBRI_COV_TEST"] = "1"
        ms, got = best_of(a.reps, lambda: ctx.coverage(key_off, key_bytes, None, ref_off, rs, rt))
        print(json.dumps({**base, "form": "uploaded", "test_before_set": True, "per_size": False, "coverage_ms": round(ms, 3), "covered_tokens": int(got[3][0][0])}), flush=True)
    if a.cli:
        with tempfile.TemporaryDirectory() as d:
            corpus, model = os.path.join(d, "probe.colibri.dat"), os.path.join(d, "probe.colibri.patternmodel")
            with open(corpus, "wb") as f:
                f.write(b"\xa2\x02" + bytes(payload))
            train = ["-f", corpus, "-l", str(a.maxlength), "-t", str(a.mintokens)]
            subprocess.run([CLI] + train + ["-o", model], capture_output=True, check=True)
            for mode in ("device", "host"):
                print(json.dumps({**base, **timed_cli(train + ["-R"], mode)}), flush=True)
                print(json.dumps({**base, **timed_cli(["-i", model, "-R"], mode)}), flush=True)


if __name__ == "__main__":
    main()
