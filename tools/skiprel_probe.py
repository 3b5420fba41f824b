"""Throughput of the three skipgram relations (getskipcontent / getinstances / gettemplates over a whole model) on one MI355X.
The model is the indexed skipgram model of a Zipf corpus (synth.zipf_corpus), trained on the device and left resident;
colibri_skipcontent_resident and colibri_relations_resident (kinds 4, 5) then run on it. Reported per call: wall time of the call (it ends with a
device synchronisation; the rows stay on the device) as the median and the spread of `--reps` runs after one warm-up (50 by default: about a second
of timed work per call), events, chunks, identity
rounds, peak scratch HBM, rows. With --host: for scale, the per-pattern host loops on the same corpus and options — colibri-patternmodeller
--skipcontent (COLIBRI_SKIPREL unset) against the same command without the flag (what training and writing the model cost), and host_selftest
skiprel_host getinstances / gettemplates against the model file's load. Prints one JSON object per line; numbers go into DESIGN.md §5h."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "colibri-core_amd", "pyhost"))
BIN = os.path.join(ROOT, "colibri-core_amd", "bin")


def timed(cmd, limit, env=None, gpu=False):
    """wall seconds of a command. Past `limit` seconds: a host-only command is given up (None) and the probe goes on; a command that opens the
    GPU ends the probe with a non-zero exit, since a slow run cannot be told from a hung device and nothing more may be started on it"""
    t0 = time.perf_counter()
    try:
        p = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=limit, env=env)
    except subprocess.TimeoutExpired:
        if gpu:
            sys.exit(f"skiprel_probe: {' '.join(cmd)} ran past {limit} s on the GPU; nothing more is started")
        return None
    if p.returncode != 0:
        raise RuntimeError(" ".join(cmd) + ": " + p.stderr[-2000:])
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=10_000_000)
    ap.add_argument("--vocab", type=int, default=100_000)
    ap.add_argument("--maxlength", type=int, default=4)
    ap.add_argument("--mintokens", type=int, default=2)
    ap.add_argument("--minskiptypes", type=int, default=2)
    ap.add_argument("--threshold", type=int, default=0)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--host", action="store_true", help="also time the per-pattern host loops")
    ap.add_argument("--host-limit", type=float, default=240.0, help="seconds after which a host-only loop is given up, and a command on the GPU ends the probe")
    a = ap.parse_args()
    from colibri_amd import capi, synth
    payload = synth.zipf_corpus(a.tokens, a.vocab, 61, header=False)
    base = {"tokens": a.tokens, "vocab": a.vocab, "maxlength": a.maxlength, "mintokens": a.mintokens, "minskiptypes": a.minskiptypes}
    with capi.Context(0) as ctx:
        ctx.upload(payload)
        st = ctx.train(mintokens=a.mintokens, maxlength=a.maxlength, indexed=1, doskipgrams=True, minskiptypes=a.minskiptypes)
        npat, _, nrefs = ctx.result_sizes()
        n, nb = capi.C.c_uint64(), capi.C.c_uint64()
        calls = (("skipcontent", lambda: ctx.L.colibri_skipcontent_resident(ctx.h, capi.C.byref(n), capi.C.byref(nb)), lambda: ctx.skipcontent_info()),
                 ("instances", lambda: ctx.L.colibri_relations_resident(ctx.h, capi.REL_INSTANCES, a.threshold, capi.C.byref(n)), lambda: ctx.relations_info() + (0, 0)),
                 ("templates", lambda: ctx.L.colibri_relations_resident(ctx.h, capi.REL_TEMPLATES, a.threshold, capi.C.byref(n)), lambda: ctx.relations_info() + (0, 0)))
        for name, call, info in calls:
            ctx._check(call())  # warm-up: code objects, the context's sort buffers
            ms = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                rc = call()
                ms.append((time.perf_counter() - t0) * 1e3)
                ctx._check(rc)
            events, chunks, scratch, rounds, skipped = info()
            med = statistics.median(ms)
            print(json.dumps(dict(base, call=name, threshold=a.threshold, patterns=npat, references=nrefs, train_ms=round(st.train_ms, 3), reps=a.reps, median_ms=round(med, 3),
                                  min_ms=round(min(ms), 3), max_ms=round(max(ms), 3), events=events, events_per_s=round(events / (med / 1e3)) if med else 0, chunks=chunks,
                                  rounds=rounds, skipped_refs=skipped, scratch_bytes=scratch, rows=n.value)), flush=True)
    if not a.host:
        return
    with tempfile.TemporaryDirectory() as tmp:
        dat, cls, model, out = (os.path.join(tmp, x) for x in ("c.colibri.dat", "c.colibri.cls", "m.colibri.patternmodel", "rows.txt"))
        with open(dat, "wb") as f:
            f.write(synth.HEADER + payload)
        with open(cls, "w") as f:
            f.write("".join(f"{i}\tw{i}\n" for i in range(6, a.vocab + 16)))
        env = {k: v for k, v in os.environ.items() if k != "COLIBRI_SKIPREL"}
        cli = [os.path.join(BIN, "colibri-patternmodeller"), "-f", dat, "-c", cls, "-s", "-l", str(a.maxlength), "-t", str(a.mintokens), "-T", str(a.minskiptypes)]
        build_s = timed(cli + ["-o", model], a.host_limit, env, gpu=True)
        print(json.dumps(dict(base, host="train + write the model (no relation)", seconds=round(build_s, 2))), flush=True)
        for flag, e in (("host", env), ("device", dict(env, COLIBRI_SKIPREL="device"))):
            s = timed(cli + ["--skipcontent"], a.host_limit, e, gpu=True)
            print(json.dumps(dict(base, host=f"--skipcontent, rows from the {flag} (train + print)", seconds=s and round(s, 2), limit=a.host_limit)), flush=True)
        selftest = os.path.join(BIN, "host_selftest")
        for fn in ("getskipcontent", "getinstances", "gettemplates"):  # host only: no device is opened
            s = timed([selftest, "skiprel_host", model, dat, fn, str(a.threshold), out], a.host_limit)
            print(json.dumps(dict(base, host=f"host_selftest skiprel_host {fn} (load + loop + write)", seconds=s and round(s, 2), limit=a.host_limit)), flush=True)


if __name__ == "__main__":
    main()
