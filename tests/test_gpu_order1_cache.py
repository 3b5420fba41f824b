"""GPU: the dense class counts of order 1 are kept between the train() calls of a context (csrc/train_api.inc order1_by_class, colibri_ctx::uni_cached).
They depend on the uploaded corpus alone, so a run on a corpus that an earlier run has counted goes straight to uni_finish_kernel. Nothing of this may show in a
model: every run here is compared with the oracle (patterns and counts, every reference list of an indexed run, found and kept per order, tokens and types), and
COLIBRI_UNI_CACHE=0 (read at every train(): every run counts again) must report the same figures. What must drop the kept counts: an upload (either entry point), a
run that failed or was repeated on the retry ladder; what must not mix: two contexts alive at once."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (mintokens, maxlength, kind): thresholds 2, 5, 1; plain, indexed, skipgrams of both kinds, plain again
RUNS = [(2, 4, {}), (5, 4, {}), (1, 3, {}), (2, 4, dict(indexed=True)), (2, 4, dict(indexed=True, doskipgrams=True)), (2, 4, dict(doskipgrams_exhaustive=True)), (2, 4, {})]
_ORACLE = {}


def _want(payload, thr, maxlength, kind):
    """one oracle model per (corpus, run), shared by the tests of this module"""
    import oracle
    key = (hash(bytes(payload)), len(payload), thr, maxlength, tuple(sorted(kind.items())))
    if key not in _ORACLE:
        _ORACLE[key] = oracle.train(bytes(payload), thr, maxlength, **kind)
    return _ORACLE[key]


def _figures(st, maxlength):
    return (st.totaltokens, st.totaltypes, st.maxn, st.npatterns, st.nrefs) + tuple((st.admitted[n], st.found[n], st.kept[n]) for n in range(1, maxlength + 1))


def _train_and_compare(ctx, payload, thr, maxlength, kind):
    want = _want(payload, thr, maxlength, kind)
    st = ctx.train(mintokens=thr, maxlength=maxlength, **{k: int(v) for k, v in kind.items()})
    got, refs = ctx.export_dict()
    assert got == want.counts, (thr, maxlength, kind, len(got), len(want.counts))
    if kind.get("indexed"):
        assert refs == want.refs, (thr, maxlength, kind)
    assert (st.totaltokens, st.totaltypes) == (want.tokens, want.types), (thr, maxlength, kind)
    for n in range(1, maxlength + 1):
        assert (st.found[n], st.kept[n]) == (want.stats[n][0], want.stats[n][2]), (thr, maxlength, kind, n)
    return _figures(st, maxlength)


@pytest.fixture(scope="module")
def corpus_a():
    from colibri_amd import synth
    return synth.zipf_corpus(60_000, 30_000, 31, header=False)  # classes beyond the LDS head of 8192: the tail bins hold tokens


def _upload(ctx, payload, device):
    """through colibri_upload_corpus, or colibri_upload_corpus_device from a tensor of the caller's"""
    if not device:
        ctx.upload(payload)
        return None
    import torch
    t = torch.from_numpy(np.frombuffer(bytes(payload), dtype=np.uint8).copy()).to("cuda:0")
    torch.cuda.synchronize()
    ctx.upload_device(t.data_ptr(), t.numel(), 1)
    return t


@pytest.mark.parametrize("device", [False, True], ids=["upload", "upload_device"])
def test_trains_in_a_row_on_one_context(corpus_a, monkeypatch, device):
    """thresholds 2, 5, 1; plain, indexed, skipgrams, plain: each model is its oracle's, and the figures are those of the same runs with every count repeated"""
    from colibri_amd import capi
    figures = {}
    for cache in ("1", "0"):
        monkeypatch.setenv("COLIBRI_UNI_CACHE", cache)
        with capi.Context(0) as ctx:
            keep = _upload(ctx, corpus_a, device)
            figures[cache] = [_train_and_compare(ctx, corpus_a, thr, maxlength, kind) for thr, maxlength, kind in RUNS]
            del keep
    assert figures["1"] == figures["0"]


@pytest.mark.parametrize("device", [False, True], ids=["upload", "upload_device"])
@pytest.mark.parametrize("b_spec", [(60_000, 30_000, 32), (20_000, 30_000, 33), (60_000, 200_000, 34)], ids=["same_length", "shorter", "larger_maxclass"])
def test_an_upload_drops_the_kept_counts(corpus_a, monkeypatch, b_spec, device):
    """upload A, train, upload B, train: B's models are B's"""
    from colibri_amd import capi, synth
    monkeypatch.delenv("COLIBRI_UNI_CACHE", raising=False)
    corpus_b = synth.zipf_corpus(*b_spec, header=False)
    with capi.Context(0) as ctx:
        keep = _upload(ctx, corpus_a, device)
        _train_and_compare(ctx, corpus_a, 2, 4, {})
        _train_and_compare(ctx, corpus_a, 2, 4, {})
        keep = _upload(ctx, corpus_b, device)
        _train_and_compare(ctx, corpus_b, 2, 4, {})
        _train_and_compare(ctx, corpus_b, 5, 4, dict(indexed=True))
        del keep


def test_overflow_route_then_ordinary_route(corpus_a, monkeypatch):
    """a run whose tail bins outgrow their room (COLIBRI_UNI_BIN_CAP, read at every train(): the tail is counted with global atomics), then runs without it"""
    from colibri_amd import capi
    monkeypatch.delenv("COLIBRI_UNI_CACHE", raising=False)
    with capi.Context(0) as ctx:
        ctx.upload(corpus_a)
        monkeypatch.setenv("COLIBRI_UNI_BIN_CAP", "8")
        a = _train_and_compare(ctx, corpus_a, 2, 4, {})
        monkeypatch.delenv("COLIBRI_UNI_BIN_CAP")
        assert _train_and_compare(ctx, corpus_a, 2, 4, {}) == a
        _train_and_compare(ctx, corpus_a, 5, 4, dict(indexed=True))
        ctx.upload(corpus_a)  # ... and the ordinary route first
        assert _train_and_compare(ctx, corpus_a, 2, 4, {}) == a
        monkeypatch.setenv("COLIBRI_UNI_BIN_CAP", "8")
        assert _train_and_compare(ctx, corpus_a, 2, 4, {}) == a


def test_two_contexts_alive_at_once(corpus_a, monkeypatch):
    from colibri_amd import capi, synth
    monkeypatch.delenv("COLIBRI_UNI_CACHE", raising=False)
    corpus_b = synth.zipf_corpus(40_000, 12_000, 35, header=False)
    with capi.Context(0) as c1, capi.Context(0) as c2:
        c1.upload(corpus_a)
        c2.upload(corpus_b)
        for thr, kind in ((2, {}), (5, {}), (2, dict(indexed=True))):
            _train_and_compare(c1, corpus_a, thr, 4, kind)
            _train_and_compare(c2, corpus_b, thr, 4, kind)
        c1.upload(corpus_b)  # one context changes its corpus, the other keeps its counts
        _train_and_compare(c1, corpus_b, 2, 4, {})
        _train_and_compare(c2, corpus_b, 2, 4, {})


def test_a_failed_and_a_repeated_run_between_good_ones(monkeypatch):
    """A train() that is refused, and one whose first attempt runs out of result room (st->overflow: duplicated text keeps more patterns than the buffers start with)
    and is repeated on the retry ladder: the runs around them are their oracles'."""
    from colibri_amd import capi, synth
    monkeypatch.delenv("COLIBRI_UNI_CACHE", raising=False)
    L, nsent = 12, 1500
    sent = np.random.default_rng(11).permutation(np.arange(6, 6 + L * nsent, dtype=np.uint32)).reshape(nsent, L)
    sym = np.concatenate([np.concatenate([sent, sent], axis=0), np.zeros((2 * nsent, 1), dtype=np.uint32)], axis=1).reshape(-1)
    dup = synth.encode_v2(sym).tobytes()
    with capi.Context(0) as ctx:
        ctx.upload(dup)
        a = _train_and_compare(ctx, dup, 2, 2, {})
        with pytest.raises(capi.ColibriError):
            ctx.train(mintokens=2, maxlength=3, minlength=2)
        assert _train_and_compare(ctx, dup, 2, 2, {}) == a
        _train_and_compare(ctx, dup, 2, L, {})
        assert ctx.stats.fallback_reason == capi.FALLBACK_RESULTS and ctx.stats.retries >= 1, "the run was meant to be repeated with more room"
        assert _train_and_compare(ctx, dup, 2, 2, {}) == a
        _train_and_compare(ctx, dup, 2, 3, dict(indexed=True))
