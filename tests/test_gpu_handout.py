"""GPU: how the count, list and bitmap kernels of the radix path hand out their work (csrc/bigram2.hpp, csrc/chain.hpp).
bi2_count_kernel draws final bins from eight queues: four at a time, and the last `tail` bins of a queue one at a time (COLIBRI_BI2_TAIL, read at every train();
0: every ticket is four bins); chain_bitmap_kernel walks a bucket's nine lists as one index space. None of this may show in the model: every run
here is compared with the oracle (patterns and counts, for indexed runs every reference list, found and kept per order).
At 2 x 10^6 tokens a queue holds 256 - 512 bins: a tail of 6 or 64 takes the mixed route (with 6 the bins that go out in fours are rounded down to a multiple of
four), the default tail — twice the waves per queue — hands every bin out singly. At 2 x 10^4 tokens most wave lists are empty and many hold one entry: lists of
length zero and tails of one to three entries in the bitmap kernel."""
import os
import pickle
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _models(payload):
    import oracle
    return {False: oracle.train(payload, 2, 5), True: oracle.train(payload, 2, 5, indexed=True)}


@pytest.fixture(scope="module")
def corpus_and_models():
    from colibri_amd import synth
    payload = synth.zipf_corpus(2_000_000, 100_000, 21, header=False)
    return payload, _models(payload)


@pytest.fixture(scope="module")
def tiny_corpus_and_models():
    from colibri_amd import synth
    payload = synth.zipf_corpus(20_000, 100_000, 22, header=False)
    return payload, _models(payload)


def _figures(st, want, maxlength=5):
    assert (st.totaltokens, st.totaltypes, st.maxn, st.npatterns) == (want.tokens, want.types, want.maxn, len(want.counts))
    for n in range(1, maxlength + 1):
        assert (st.found[n], st.kept[n]) == (want.stats[n][0], want.stats[n][2]), n


def _single_device(payload, want, indexed):
    from colibri_amd import capi
    with capi.Context(0) as ctx:
        ctx.upload(payload)
        st = ctx.train(mintokens=2, maxlength=5, indexed=int(indexed))
        got, refs = ctx.export_dict()
    assert st.path & capi.PATH_CHAIN and st.retries == 0, ("the chained orders must have run, once", st.path, st.retries, st.fallback_reason)
    assert got == want.counts
    if indexed:
        assert refs == want.refs
    _figures(st, want)


@pytest.mark.parametrize("tail", ["0", "6", "64", None], ids=["tail0", "tail6", "tail64", "default"])
@pytest.mark.parametrize("indexed", [False, True], ids=["plain", "indexed"])
def test_bin_handout(corpus_and_models, monkeypatch, indexed, tail):
    payload, models = corpus_and_models
    if tail is None:
        monkeypatch.delenv("COLIBRI_BI2_TAIL", raising=False)
    else:
        monkeypatch.setenv("COLIBRI_BI2_TAIL", tail)
    _single_device(payload, models[indexed], indexed)


def test_wide_form(corpus_and_models, tmp_path):
    """the 2048-slot tables and eight sub-regions of corpora beyond 2.15 x 10^8 positions (COLIBRI_FORCE_WIDE_CHAIN is read once per process: a child process)"""
    payload, models = corpus_and_models
    want = models[False]
    job = tmp_path / "job.pkl"
    with open(job, "wb") as f:
        pickle.dump({"payload": bytes(payload), "counts": want.counts, "figures": (want.tokens, want.types, want.maxn), "stats": {n: tuple(want.stats[n]) for n in range(1, 6)}}, f)
    env = dict(os.environ, COLIBRI_FORCE_WIDE_CHAIN="1")
    env.pop("COLIBRI_BI2_TAIL", None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "handout_worker.py"), str(job)], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0 and "HANDOUT_OK" in p.stdout, p.stdout[-2000:] + p.stderr[-3000:]


def test_key_sharded_owners(corpus_and_models, monkeypatch):
    """the owners' forms of the same loop (records are 4-byte keys, the lists are chunks of a pool)"""
    from colibri_amd import capi
    monkeypatch.delenv("COLIBRI_BI2_TAIL", raising=False)
    payload, models = corpus_and_models
    with capi.ShardedTrainer(2, devices=[0, 0]) as tr:
        tr.upload_split(payload)
        st = tr.train(mintokens=2, maxlength=5)
        assert tr.info.protocol == 0, "the run did not take the key-sharded path"
        got = tr.export_dict()
    assert got == models[False].counts
    _figures(st, models[False])


@pytest.mark.parametrize("indexed", [False, True], ids=["plain", "indexed"])
def test_near_empty_lists(tiny_corpus_and_models, monkeypatch, indexed):
    monkeypatch.delenv("COLIBRI_BI2_TAIL", raising=False)
    payload, models = tiny_corpus_and_models
    _single_device(payload, models[indexed], indexed)
