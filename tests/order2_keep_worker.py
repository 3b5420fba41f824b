"""Worker of tests/test_gpu_order2_keep.py for the switches the library reads once per process: COLIBRI_FORCE_WIDE_CHAIN (mode "wide": the kept partition is
reused by runs whose orders >= 3 take the wide form) and COLIBRI_SLICE_POSITIONS (mode "sliced": an order counted in passes over key slices is not kept).
Every run is compared with the oracle, and the sequence's figures with those of the same sequence under COLIBRI_BI2_KEEP=0."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "colibri-core_amd", "pyhost"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from colibri_amd import capi  # noqa: E402
from test_gpu_order2_keep import corpus, run_sequence  # noqa: E402


def main():
    mode = sys.argv[1]
    assert os.environ.get({"wide": "COLIBRI_FORCE_WIDE_CHAIN", "sliced": "COLIBRI_SLICE_POSITIONS"}[mode])
    payload = corpus("phrases")
    runs = [(2, 5, {}), (2, 5, {}), (2, 4, dict(indexed=True))] if mode == "wide" else [(2, 5, {}), (2, 5, {}), (2, 3, {})]
    figures = {}
    for keep in ("1", "0"):
        os.environ["COLIBRI_BI2_KEEP"] = keep
        with capi.Context(0) as ctx:
            ctx.upload(payload)
            figures[keep], reused = run_sequence(ctx, payload, runs, sliced=mode == "sliced")
            if mode == "wide":
                assert ctx.stats.path & capi.PATH_WIDE, ctx.stats.path
                assert reused == ([False, True, True] if keep == "1" else [False] * 3), (keep, reused)
            else:
                assert ctx.last_mode(True)[1] > 1, ctx.last_mode(True)
                assert reused == [False] * 3, (keep, reused)
    assert figures["1"] == figures["0"]
    print("KEEP_OK")


if __name__ == "__main__":
    main()
