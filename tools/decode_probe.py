"""Corpus decoding at scale: a Zipf corpus of --tokens tokens (vocab --vocab, the bench family's generator), decoded
  * through ctx.decode into a null sink (best of --reps, wall time of the whole call: upload, tokenise, table, kernels, copies),
  * by colibri-classdecode to /dev/null and to a file (wall time of the process),
and the bytes the kernels must move: the payload read once, the text written once (the D2H copy reads it again).

  python tools/decode_probe.py [--tokens N] [--vocab V] [--reps R] [--dir D] [--kernels-only] [--ref BINARY]

--kernels-only runs one ctx.decode and nothing else (for `rocprofv3 --kernel-trace --stats -- python tools/decode_probe.py --kernels-only`).
--ref times another colibri-classdecode binary (the reference's, built elsewhere) on the same files. Prints one JSON line."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "colibri-core_amd", "pyhost"))
CLI = os.path.join(ROOT, "colibri-core_amd", "bin", "colibri-classdecode")


class _NoDevice:
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=100_000_000)
    ap.add_argument("--vocab", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dir", default=None, help="where the corpus, class file and text go while timed (default: a fresh temporary directory)")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--ref", default=None)
    ap.add_argument("--no-device", action="store_true", help="time --ref only (a host without a GPU)")
    a = ap.parse_args()
    from colibri_amd import capi, synth
    own_dir = a.dir is None
    a.dir = a.dir or tempfile.mkdtemp(prefix="decode_probe_")
    os.makedirs(a.dir, exist_ok=True)
    t0 = time.perf_counter()
    payload = synth.zipf_corpus(a.tokens, a.vocab, 5, header=False)
    gen_s = time.perf_counter() - t0
    words = {i: f"w{i}".encode() for i in range(6, a.vocab + 6)}
    res = {"tokens": a.tokens, "vocab": a.vocab, "payload_bytes": len(payload), "generate_s": round(gen_s, 2)}
    with (capi.Context(0) if not a.no_device else _NoDevice()) as ctx:
        if ctx is None:
            pass
        elif a.kernels_only:
            n = [0]
            ctx.decode(words, payload, sink=lambda m: n.__setitem__(0, n[0] + len(m)))
            res["text_bytes"] = n[0]
            if own_dir:
                os.rmdir(a.dir)
            print(json.dumps(res))
            return
        best = None
        for _ in range(a.reps if ctx is not None else 0):
            n = [0]
            t = time.perf_counter()
            ctx.decode(words, payload, sink=lambda m: n.__setitem__(0, n[0] + len(m)))
            dt = time.perf_counter() - t
            best = dt if best is None else min(best, dt)
        if ctx is not None:
            res["text_bytes"] = n[0]
            res["ctx_decode_null_sink_s"] = round(best, 3)
            res["windows"], res["staging_bytes"], res["scratch_bytes"] = ctx.decode_info()
            res["algorithmic_bytes"] = len(payload) + res["text_bytes"]  # payload read once + text written once
    dat, cls, out = (os.path.join(a.dir, f) for f in ("zipf.colibri.dat", "zipf.colibri.cls", "zipf.txt"))
    with open(dat, "wb") as f:
        f.write(synth.HEADER + payload)
    with open(cls, "w") as f:
        f.write("".join(f"{i}\tw{i}\n" for i in range(6, a.vocab + 6)))

    def timed(binary, target):
        with open(target, "wb") as f:
            t = time.perf_counter()
            r = subprocess.run([binary, "-c", cls, "-f", dat], stdout=f, stderr=subprocess.PIPE, timeout=1200)
            dt = time.perf_counter() - t
        if r.returncode != 0:
            raise SystemExit(r.stderr.decode()[-2000:])
        return round(dt, 3)
    for name, binary in (("cli", None if a.no_device else CLI), ("ref", a.ref)):
        if binary:
            res[f"{name}_devnull_s"] = timed(binary, os.devnull)
            res[f"{name}_file_s"] = timed(binary, out)
            res[f"{name}_file_bytes"] = os.path.getsize(out)
    for p in (dat, cls, out):
        if os.path.exists(p):
            os.remove(p)
    if own_dir:
        os.rmdir(a.dir)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
