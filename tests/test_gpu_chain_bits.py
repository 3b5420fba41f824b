"""GPU: chain_emit_kernel's successor test — "did the (n-1)-gram at i + 1 survive" — in its three forms (csrc/chain.hpp, the launches in csrc/colibri_hip.hip and
csrc/kshard_api.inc): the bucket's slice of the bitmap in LDS, copied when a block's run of steps reaches another bucket (the form of every corpus whose position
buckets hold at most 2^17 positions); the gather from memory (COLIBRI_CH_BITS_LDS=0, read at every launch: the form of larger buckets, the kernel as it was);
and the LDS form beside records that lack three position bits (COLIBRI_FORCE_WIDE_CHAIN=1, read once per process: a child process).

The corpora are BUILT (tests/chain_bits_models.py, run on the host by tests/test_chain_step.py) so that every edge of the LDS form occurs, and the builder asserts
that it does: surviving (n-1)-grams at a bucket's last position with a surviving and with a pruned successor in the next bucket for n = 3, 4, 5, the same for head
windows of order 2, a list of two steps between empty buckets, runs of steps that cross a bucket change, an XCD with a single step, a partial last bucket that ends
in a surviving 5-gram, and slices of every length modulo four. Every run trains through the C ABI and is held to the oracle's model of the same payload — patterns
and counts, every reference of an indexed model, found / pruned / kept per order — and to the corpus' census of the windows each order admits; the forms must also
agree on the windows they report per order. Equality throughout."""
import functools
import json
import os
import subprocess
import sys

import pytest

import chain_bits_models as cb
from conftest import ROOT

pytestmark = pytest.mark.gpu

FIGURES = ("windows", "admitted", "found", "pruned", "kept")


@pytest.fixture(scope="module")
def ctx():
    from colibri_amd import capi
    with capi.Context(0) as c:
        yield c


_case = functools.lru_cache(maxsize=None)(cb.edges)


@functools.lru_cache(maxsize=None)
def _oracle(last, indexed, long=4000):
    import oracle
    return oracle.train(_case(last, long).corpus.payload, 2, 5, indexed=indexed)


def hold(case, want, figures, what):
    """the per-order figures of a run against the oracle's and the corpus' census"""
    for n in range(1, 6):
        assert (figures["found"][n - 1], figures["pruned"][n - 1], figures["kept"][n - 1]) == want.stats[n], (what, n)
    for n in range(2, 6):
        assert figures["admitted"][n - 1] == case.admitted[n], (what, n, figures["admitted"], case.admitted)
    assert sum(figures["windows"]) == want.windows, what


def train(ctx, last, indexed, what):
    from colibri_amd import capi
    case, want = _case(last), _oracle(last, indexed)
    ctx.upload(case.corpus.payload)
    assert ctx.positions() == case.corpus.npos
    st = ctx.train(mintokens=2, maxlength=5, indexed=int(indexed))
    got, refs = ctx.export_dict()
    assert got == want.counts, what
    if indexed:
        assert refs == want.refs, what
    assert (st.totaltokens, st.totaltypes, st.maxn, st.npatterns) == (want.tokens, want.types, 5, len(want.counts)), what
    assert (st.fallback_reason, st.retries) == (0, 0) and st.path & capi.PATH_BI2 and st.path & capi.PATH_CHAIN and not st.path & capi.PATH_WIDE, (what, st.path)
    figures = {k: [int(getattr(st, k)[n]) for n in range(1, 6)] for k in FIGURES}
    hold(case, want, figures, what)
    return figures


@pytest.mark.parametrize("indexed", [False, True], ids=["plain", "indexed"])
def test_every_edge_in_lds_and_by_gather(ctx, monkeypatch, indexed):
    """the slice in LDS, then the same corpus with COLIBRI_CH_BITS_LDS=0: both the oracle's model, and the same figures per order"""
    monkeypatch.delenv("COLIBRI_CH_BITS_LDS", raising=False)
    lds = train(ctx, 577, indexed, "lds")
    monkeypatch.setenv("COLIBRI_CH_BITS_LDS", "0")
    gather = train(ctx, 577, indexed, "gather")
    monkeypatch.setenv("COLIBRI_CH_BITS_LDS", "1")  # (only "0" turns it off)
    again = train(ctx, 577, indexed, "lds again")
    assert lds == gather == again


@pytest.mark.parametrize("last", [545, 609])
def test_slices_of_every_length_modulo_four(ctx, monkeypatch, last):
    """the last bucket's slice ends with the bitmap: 34 and 36 words here, 35 in the corpus above, 129 for every full bucket — 16-byte groups and 0 .. 3 single words"""
    monkeypatch.delenv("COLIBRI_CH_BITS_LDS", raising=False)
    assert _case(last).slice_words[0] in (34, 36)
    train(ctx, last, False, "lds")


def test_wide_form_in_a_child_process():
    """COLIBRI_FORCE_WIDE_CHAIN=1: eight sub-regions and dropped position bits beside the LDS slice (the buckets still hold 4096 positions); plain and indexed.
    The same corpus with its long sentences cut to 1800 and 1350 tokens: the wide form's record slots are half as large, and a hot key's 3999 records in one of them
    make the run give the chained orders up (FALLBACK_CHAIN: the right model, by other kernels)"""
    env = dict(os.environ, COLIBRI_FORCE_WIDE_CHAIN="1")
    env.pop("COLIBRI_CH_BITS_LDS", None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "chain_bits_worker.py"), "577", "1800"], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    out = json.loads([line for line in p.stdout.splitlines() if line.startswith("CHAIN_BITS ")][-1][len("CHAIN_BITS "):])
    for kind, indexed in (("plain", False), ("indexed", True)):
        hold(_case(577, 1800), _oracle(577, indexed, 1800), out[kind], "wide " + kind)


def test_key_sharded_two_ranks_on_one_device():
    """the key-sharded trainer's launch of the same kernel takes the same choice: two ranks on one device, the oracle's model (the corpus of the wide form: the
    key-sharded trainer has its record slots)"""
    from colibri_amd import capi
    case, want = _case(577, 1800), _oracle(577, False, 1800)
    with capi.ShardedTrainer(2, devices=[0, 0]) as tr:
        tr.upload_split(case.corpus.payload)
        st = tr.train(mintokens=2, maxlength=5)
        got = tr.export_dict()
        assert tr.info.protocol == 0, "the run did not take the key-sharded path"
    assert got == want.counts
    assert (st.totaltokens, st.totaltypes, st.maxn, st.npatterns) == (want.tokens, want.types, 5, len(want.counts))
    for n in range(1, 6):
        assert (st.found[n], st.kept[n]) == (want.stats[n][0], want.stats[n][2]), n
