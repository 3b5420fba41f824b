"""Worker of tests/test_gpu_handout.py: trains the corpus of the pickled job in a process of its own (the environment holds a switch the library reads once
per process) and compares the model with the expected one the job carries."""
import os
import pickle
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "colibri-core_amd", "pyhost"))

from colibri_amd import capi  # noqa: E402


def main():
    with open(sys.argv[1], "rb") as f:
        job = pickle.load(f)
    with capi.Context(0) as ctx:
        ctx.upload(job["payload"])
        st = ctx.train(mintokens=2, maxlength=5)
        got, _ = ctx.export_dict()
    if os.environ.get("COLIBRI_FORCE_WIDE_CHAIN"):
        assert st.path & capi.PATH_WIDE, ("the wide form of the chained orders must have run", st.path)
    assert st.path & capi.PATH_CHAIN and st.retries == 0, (st.path, st.retries, st.fallback_reason)
    assert got == job["counts"], (len(got), len(job["counts"]))
    assert (st.totaltokens, st.totaltypes, st.maxn) == job["figures"]
    for n in range(1, 6):
        assert (st.found[n], st.kept[n]) == (job["stats"][n][0], job["stats"][n][2]), n
    print("HANDOUT_OK")


if __name__ == "__main__":
    main()
