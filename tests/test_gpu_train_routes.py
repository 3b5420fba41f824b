"""The routes of colibri_train: every kind of run, under every environment switch that can change which loop and which engines it takes, against the oracle AND
against what the training driver did before it was taken apart into a mode plan, three order loops and one retry ladder.

The second comparison is a table (train_routes_expected.json) recorded once from the library of the commit before that change — `python tests/test_gpu_train_routes.py`
against such a build — and never regenerated since: the engines that ran (path), the repeats, the counting mode, the per-order figures and the number of profiled
brackets per kernel class (Prof scopes, not launches: it pins where every scope begins and ends).
"""
import json
import os

import pytest

from conftest import small_corpora

pytestmark = pytest.mark.gpu

EXPECTED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "train_routes_expected.json")
CORPORA = ("zipf200k_phrases", "zipf20k")
NCLASSES = 15  # COLIBRI_K_NCLASSES
KINDS = {
    "plain": dict(),
    "plain_table": dict(table_mode=1),
    "plain_radix": dict(table_mode=2),
    "maxlength2": dict(maxlength=2),
    "indexed": dict(indexed=1),
    "indexed_skip": dict(indexed=1, doskipgrams=1),
    "indexed_skip_types2": dict(indexed=1, doskipgrams=1, minskiptypes=2),
    "indexed_skip_types1": dict(indexed=1, doskipgrams=1, minskiptypes=1),
    "exhaustive": dict(doskipgrams_exhaustive=1),
    "unigram_threshold": dict(mintokens_unigrams=5),
    "mintokens1": dict(mintokens=1),
    "backoff2": dict(maxbackofflength=2),
}
_ID_KEEPING = ("indexed", "indexed_skip", "indexed_skip_types2", "indexed_skip_types1", "exhaustive")
# a switch is tried on the kinds whose mode plan reads it
SWITCHES = {
    "COLIBRI_NO_CHAIN": ("plain", "unigram_threshold", "mintokens1") + _ID_KEEPING,
    "COLIBRI_NO_CHAIN_IDS": _ID_KEEPING,
    "COLIBRI_ALL_IDS": _ID_KEEPING,
    "COLIBRI_SYNCED_LOOP": _ID_KEEPING,
    "COLIBRI_SYNCED_SKIPS": ("indexed_skip", "indexed_skip_types2", "indexed_skip_types1"),
    "COLIBRI_NO_DIRECT_PAIRS": ("indexed", "indexed_skip", "indexed_skip_types2", "indexed_skip_types1"),
    "COLIBRI_NO_SKIP_CHAIN": ("exhaustive",),
}
CASES = [(corpus, kind, "") for corpus in CORPORA for kind in KINDS] + [(corpus, kind, sw) for corpus in CORPORA for sw, kinds in SWITCHES.items() for kind in kinds]

_oracle = {}


def _want(corpus, kind):
    """the oracle's model of a kind: computed once, shared by the switches (which must not change it) and by the table modes"""
    import oracle
    opts = dict(mintokens=2, maxlength=5)
    opts.update({k: v for k, v in KINDS[kind].items() if k != "table_mode"})
    key = (corpus, tuple(sorted(opts.items())))
    if key not in _oracle:
        _oracle[key] = oracle.train(small_corpora()[corpus], opts.pop("mintokens"), opts.pop("maxlength"), **opts)
    return _oracle[key]


def _run(ctx, corpus, kind):
    """one training run -> (counts, references, the route it took)"""
    opts = dict(mintokens=2, maxlength=5, profile=1)
    opts.update(KINDS[kind])
    ctx.upload(small_corpora()[corpus])
    st = ctx.train(**opts)
    counts, refs = ctx.export_dict()
    route = {
        "path": st.path, "retries": st.retries, "fallback_reason": st.fallback_reason, "last_mode": list(ctx.last_mode(with_passes=True)),
        "found": list(st.found[1:6]), "kept": list(st.kept[1:6]), "admitted": list(st.admitted[1:6]),
        "brackets": [int(ctx.kernel_time(cls)[1]) for cls in range(NCLASSES)],
    }
    return counts, refs, route


@pytest.fixture(scope="module")
def ctx():
    from colibri_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def expected():
    with open(EXPECTED) as f:
        return json.load(f)


@pytest.mark.parametrize("corpus,kind,switch", CASES, ids=["-".join(x for x in case if x) for case in CASES])
def test_route_and_model(ctx, expected, monkeypatch, corpus, kind, switch):
    if switch:
        monkeypatch.setenv(switch, "1")  # (the driver reads these at every call)
    counts, refs, route = _run(ctx, corpus, kind)
    want = _want(corpus, kind)
    assert counts == want.counts, "pattern set / counts differ from the oracle"
    if KINDS[kind].get("indexed"):
        assert refs == want.refs, "references differ from the oracle"
    assert route == expected["|".join((corpus, kind, switch))]


if __name__ == "__main__":  # record the table: only ever against a build of the commit before the driver was taken apart
    import sys
    from colibri_amd import capi
    table = {}
    with capi.Context(0) as c:
        for corpus, kind, switch in CASES:
            if switch:
                os.environ[switch] = "1"
            try:
                table["|".join((corpus, kind, switch))] = _run(c, corpus, kind)[2]
            finally:
                os.environ.pop(switch, None)
    with open(sys.argv[1] if len(sys.argv) > 1 else EXPECTED, "w") as f:
        json.dump(table, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(table)} routes")
