"""N-gram extraction at scale: a Zipf corpus of 10^7 tokens (vocab 50 000, seed 91, the bench family's generator), n = 3, through the C ABI
with a sink that only counts, and colibri_decode of the same corpus through the same output pump for comparison.

  python tools/ngrams_probe.py e2e            one warm-up, then 7 alternating repeats of each; medians and ranges as one JSON object
                                              (call = colibri_ngrams / colibri_decode alone, with_upload = upload and word table included); also the
                                              SHA-256 of the whole text
  python tools/ngrams_probe.py kernels        four calls and nothing else: rocprofv3 --kernel-trace --stats -- python tools/ngrams_probe.py kernels
  python tools/ngrams_probe.py gen DIR        DIR/zipf10m.payload (the data without A2 02) and DIR/zipf10m.colibri.cls, for another colibri-extractngrams
                                              binary (the reference's, built elsewhere): time BINARY -c ...cls -n 3 ...payload > /dev/null"""
import ctypes as C
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "colibri-core_amd", "pyhost"))
import numpy as np  # noqa: E402
from colibri_amd import capi, synth  # noqa: E402

NTOK, VOCAB, SEED, N = 10_000_000, 50_000, 91, 3


def corpus():
    payload = np.frombuffer(synth.zipf_corpus(NTOK, VOCAB, SEED, header=False), dtype=np.uint8)
    words = {i: f"w{i}".encode() for i in range(6, VOCAB + 6)} | {1: b"{|}", 2: b"{?}", 3: b"{*}", 4: b"{**}"}
    return payload, words


class Counter:
    def __init__(self):
        self.n = 0
        self.cb = capi.DecodeSink(self.take)

    def take(self, _user, _p, n):
        self.n += n
        return 0


def ngrams_once(ctx, payload, words):
    cnt = Counter()
    nb, ng = C.c_uint64(), C.c_uint64()
    t0 = time.perf_counter()
    ctx._check(ctx.L.colibri_decode_upload(ctx.h, payload.ctypes.data, payload.size, 2, None))
    ctx._print_classes(words)
    t1 = time.perf_counter()
    ctx._check(ctx.L.colibri_ngrams(ctx.h, N, cnt.cb, None, C.byref(nb), C.byref(ng)))  # (returns after the last window was handed over)
    t2 = time.perf_counter()
    assert cnt.n == nb.value
    return {"call_ms": (t2 - t1) * 1e3, "with_upload_ms": (t2 - t0) * 1e3, "bytes": nb.value, "rows": ng.value}


def decode_once(ctx, payload, words):
    cnt = Counter()
    nb, nl, mc = C.c_uint64(), C.c_uint64(), C.c_uint64()
    t0 = time.perf_counter()
    ctx._check(ctx.L.colibri_decode_upload(ctx.h, payload.ctypes.data, payload.size, 2, C.byref(mc)))
    nids = min(max(words), mc.value) + 1
    kept = sorted(k for k in words if k < nids)
    lens = np.zeros(nids, dtype=np.uint64)
    lens[kept] = [len(words[k]) for k in kept]
    off = np.zeros(nids + 1, dtype=np.uint64)
    np.cumsum(lens, out=off[1:])
    wb = np.frombuffer(b"".join(words[k] for k in kept) + b"\0", dtype=np.uint8)
    ctx._check(ctx.L.colibri_decode_classes(ctx.h, off.ctypes.data, wb.ctypes.data, nids))
    t1 = time.perf_counter()
    ctx._check(ctx.L.colibri_decode(ctx.h, 0, 0, cnt.cb, None, C.byref(nb), C.byref(nl)))
    t2 = time.perf_counter()
    return {"call_ms": (t2 - t1) * 1e3, "with_upload_ms": (t2 - t0) * 1e3, "bytes": nb.value, "rows": nl.value}


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "e2e"
    payload, words = corpus()
    if mode == "gen":
        open(os.path.join(sys.argv[2], "zipf10m.payload"), "wb").write(payload.tobytes())
        open(os.path.join(sys.argv[2], "zipf10m.colibri.cls"), "w").write("".join(f"{i}\tw{i}\n" for i in range(6, VOCAB + 6)))
        return
    with capi.Context(0) as ctx:
        if mode == "kernels":
            for _ in range(4):
                r = ngrams_once(ctx, payload, words)
            print(json.dumps(r))
            return
        h = hashlib.sha256()
        ctx.ngrams(words, payload, N, sink=h.update)
        runs = {"ngrams": [], "decode": []}
        ngrams_once(ctx, payload, words)  # warm-up
        decode_once(ctx, payload, words)
        for _ in range(7):  # alternating
            runs["ngrams"].append(ngrams_once(ctx, payload, words))
            runs["decode"].append(decode_once(ctx, payload, words))
        out = {"sha256": h.hexdigest(), "tokens": NTOK, "vocab": VOCAB, "seed": SEED, "n": N, "payload_bytes": int(payload.size)}
        for k, rs in runs.items():
            call = sorted(r["call_ms"] for r in rs)
            full = sorted(r["with_upload_ms"] for r in rs)
            out[k] = {"bytes": rs[0]["bytes"], "rows": rs[0]["rows"], "call_ms": [call[len(call) // 2], call[0], call[-1]], "with_upload_ms": [full[len(full) // 2], full[0], full[-1]],
                      "GB_per_s": rs[0]["bytes"] / call[len(call) // 2] / 1e6}
        print(json.dumps(out))


main()
