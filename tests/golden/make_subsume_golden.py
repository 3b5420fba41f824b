"""Generates the subsumption-prune fixtures of tests/test_subsume.py by running the REAL reference (oracle/_ref/ref_driver, built by
oracle/Makefile's `ref` rule) — run in the build container only:  python tests/golden/make_subsume_golden.py

Inputs (committed): hamlet.v2.colibri.dat, zipf20k.colibri.dat.
Outputs: subsumption.<corpus>.<us|is>.<p4|S3|p5S5>.txt — canonical dumps of the reference's skipgram models after PRUNENONSUBSUMED = 4,
PRUNESUBSUMED = 3, and both at 5 (l = 5, t = 2); subsumption.levels.json — for these and for the n-gram goldens make_golden.py writes
(subsumption.<corpus>.<u|i>.<p4|S3>.txt), the per-level lines the reference prints on stderr without -q: [pass, tokens of the pruned
patterns, patterns pruned], in the order printed.
Every run is made twice; a dump or a list of levels that differs between the two runs stops the script (the reference's skipgram loop of
an indexed model inserts into the map it iterates, include/patternmodel.h:2986-2991)."""
import json
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import oracle  # noqa: E402

DRIVER = oracle.REF_DRIVER
FLAGS = {"p4": ["-p", "4"], "S3": ["-S", "3"], "p5S5": ["-p", "5", "-S", "5"]}
LINE = re.compile(r"^ pruned (\d+) (non-subsumed|subsumed) (\d+)-grams$")


def run(corpus, mode, tag, dump):
    """one reference run without -q: the dump is written, the levels come back"""
    cmd = [DRIVER, "train", os.path.join(HERE, f"{corpus}.colibri.dat"), mode, "5", "2"] + FLAGS[tag] + ["-d", dump]
    err = subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True).stderr
    levels = []
    for ln in err.splitlines():
        m = LINE.match(ln)
        if m:
            levels.append([1 if m.group(2) == "non-subsumed" else 2, int(m.group(3)), int(m.group(1))])
    return levels


def main():
    levels = {}
    with tempfile.TemporaryDirectory() as d:
        for corpus in ("hamlet.v2", "zipf20k"):
            for mode, tags in (("u", ("p4", "S3")), ("i", ("p4", "S3")), ("us", tuple(FLAGS)), ("is", tuple(FLAGS))):
                for tag in tags:
                    a, b = os.path.join(d, "a.txt"), os.path.join(d, "b.txt")
                    la, lb = run(corpus, mode, tag, a), run(corpus, mode, tag, b)
                    ta, tb = open(a).read(), open(b).read()
                    if ta != tb or la != lb:
                        sys.exit(f"{corpus} {mode} {tag}: two runs of the reference differ")
                    name = f"subsumption.{corpus}.{mode}.{tag}.txt"
                    if mode in ("us", "is"):
                        with open(os.path.join(HERE, name), "w") as f:
                            f.write(ta)
                    elif open(os.path.join(HERE, name)).read() != ta:
                        sys.exit(f"{name}: the committed golden is not what the reference writes now")
                    levels[f"{corpus}.{mode}.{tag}"] = la
    with open(os.path.join(HERE, "subsumption.levels.json"), "w") as f:
        f.write("{\n" + ",\n".join(f' "{k}": {json.dumps(levels[k])}' for k in sorted(levels)) + "\n}\n")  # one run per line
    print("subsumption fixtures written:", len(levels), "runs")


if __name__ == "__main__":
    main()
