"""Worker of tests/test_gpu_chain_bits.py for COLIBRI_FORCE_WIDE_CHAIN, which the library reads once per process: trains the edge corpus (plain and indexed) through
the wide form of the chained orders — eight sub-regions, records whose position lacks three bits —, compares each model with the oracle's and prints the per-order
figures for the parent to hold against the corpus' census. Arguments: the corpus' last bucket and longest sentence (chain_bits_models.edges)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "colibri-core_amd", "pyhost"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import oracle  # noqa: E402
from colibri_amd import capi  # noqa: E402

import chain_bits_models as cb  # noqa: E402


def main():
    assert os.environ.get("COLIBRI_FORCE_WIDE_CHAIN")
    case = cb.edges(int(sys.argv[1]), int(sys.argv[2]))
    out = {}
    with capi.Context(0) as ctx:
        ctx.upload(case.corpus.payload)
        for indexed in (False, True):
            want = oracle.train(case.corpus.payload, 2, 5, indexed=indexed)
            st = ctx.train(mintokens=2, maxlength=5, indexed=int(indexed))
            got, refs = ctx.export_dict()
            assert got == want.counts, ("model", indexed)
            assert not indexed or refs == want.refs, "references"
            assert st.path & capi.PATH_CHAIN and st.path & capi.PATH_WIDE and (st.fallback_reason, st.retries) == (0, 0), (st.path, st.fallback_reason, st.retries)
            out["indexed" if indexed else "plain"] = {k: [int(getattr(st, k)[n]) for n in range(1, 6)] for k in ("windows", "admitted", "found", "pruned", "kept")}
    print("CHAIN_BITS " + json.dumps(out))


if __name__ == "__main__":
    main()
