"""Throughput of the log-likelihood model comparison (colibri-comparemodels; colibri_compare) on one MI355X.
--models Zipf corpora (synth.zipf_corpus, one seed each) of --tokens / --models tokens are trained on the device (unindexed, MINTOKENS /
MAXLENGTH as given) and exported. Reported: the wall time of colibri_compare to its end (it ends with a device synchronisation;
the rows stay on the device; best of --reps, sorted and -a), the fetch of the rows, distinct patterns, rows, peak scratch HBM; with --cli,
the models are written to files and colibri-comparemodels is timed end to end (load, device call, print to /dev/null). Prints one JSON object
per line; numbers go into DESIGN.md."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "colibri-core_amd", "pyhost"))
CLI = os.path.join(ROOT, "colibri-core_amd", "bin", "colibri-comparemodels")


def write_model(path, tokens, key_off, key_bytes, counts):
    """an unindexed .colibri.patternmodel (00, type 10, version 2, u64 tokens, u64 types, u64 patterns, then key 00 count per pattern)"""
    n = len(counts)
    off = key_off.astype(np.int64)
    lens = np.diff(off)
    rec = lens + 5  # key, 00, u32 count
    start = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(rec, out=start[1:])
    body = np.zeros(int(start[-1]), dtype=np.uint8)
    kb = np.asarray(key_bytes, dtype=np.uint8)[: int(off[-1])]
    body[np.repeat(start[:-1] - off[:-1], lens) + np.arange(int(off[-1]))] = kb
    c4 = counts.astype("<u4").view(np.uint8).reshape(-1, 4)
    for b in range(4):
        body[start[:-1] + lens + 1 + b] = c4[:, b]
    with open(path, "wb") as f:
        f.write(bytes([0, 10, 2]) + np.array([tokens, 0, n], dtype="<u8").tobytes())
        f.write(body.tobytes())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=10_000_000)
    ap.add_argument("--models", type=int, default=2)
    ap.add_argument("--vocab", type=int, default=100_000)
    ap.add_argument("--maxlength", type=int, default=3)
    ap.add_argument("--mintokens", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cli", action="store_true")
    a = ap.parse_args()
    from colibri_amd import capi, synth
    models = []
    with capi.Context(0) as ctx:
        for m in range(a.models):
            ctx.upload(synth.zipf_corpus(a.tokens // a.models, a.vocab, 71 + m, header=False))
            st = ctx.train(mintokens=a.mintokens, maxlength=a.maxlength)
            key_off, key_bytes, counts, _ = ctx.export_arrays()
            models.append((key_off, key_bytes, counts, st.totaltokens))
        npat = sum(len(m[2]) for m in models)
        for conj in (False, True):
            flags = capi.COMPARE_CONJUNCTION if conj else 0
            P = capi.C.c_void_p * a.models
            offs, kbs, cnts = P(*[m[0].ctypes.data for m in models]), P(*[m[1].ctypes.data for m in models]), P(*[m[2].ctypes.data for m in models])
            npa = np.array([len(m[2]) for m in models], dtype=np.uint64)
            tok = np.array([m[3] for m in models], dtype=np.uint64)
            best, rows = None, 0
            for _ in range(a.reps):
                n = capi.C.c_uint64()
                t0 = time.perf_counter()
                rc = ctx.L.colibri_compare(ctx.h, a.models, offs, kbs, cnts, npa.ctypes.data, tok.ctypes.data, flags, capi.C.byref(n))
                ms = (time.perf_counter() - t0) * 1e3
                ctx._check(rc)
                best, rows = (ms if best is None else min(best, ms)), n.value
            t0 = time.perf_counter()
            K, N = rows, a.models
            bufs = [np.zeros(max(1, K), dtype=np.uint32), np.zeros(max(1, K), dtype=np.uint32), np.zeros(max(1, K), dtype=np.float64),
                    np.zeros(max(1, K * N), dtype=np.uint32), np.zeros(max(1, K * N), dtype=np.uint32)]
            ctx._check(ctx.L.colibri_compare_fetch(ctx.h, *[b.ctypes.data for b in bufs]))
            fetch_ms = (time.perf_counter() - t0) * 1e3
            distinct, scratch = ctx.compare_info()
            print(json.dumps({"tokens": a.tokens, "models": a.models, "vocab": a.vocab, "maxlength": a.maxlength, "mintokens": a.mintokens, "conjunction": conj,
                              "patterns_in": npat, "distinct": distinct, "rows": rows, "compare_ms": round(best, 3), "fetch_ms": round(fetch_ms, 3),
                              "scratch_bytes": scratch}), flush=True)
    if a.cli:
        with tempfile.TemporaryDirectory() as d:
            files = []
            for m, (ko, kb, ct, tk) in enumerate(models):
                files.append(os.path.join(d, f"m{m}.colibri.patternmodel"))
                write_model(files[-1], tk, ko, kb, ct)
            cls = os.path.join(d, "empty.colibri.cls")
            open(cls, "w").close()
            for opts in ([], ["-a"], ["-d"]):
                t0 = time.perf_counter()
                r = subprocess.run([CLI, "-c", cls] + opts + files, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=1200)
                s = time.perf_counter() - t0
                assert r.returncode == 0, r.stderr[-2000:]
                print(json.dumps({"tokens": a.tokens, "models": a.models, "cli": opts, "cli_s": round(s, 3)}), flush=True)


if __name__ == "__main__":
    main()
