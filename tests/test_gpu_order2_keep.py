"""GPU: order 2's partition is kept between the train() calls of a context (csrc/colibri_hip.hip bigram2_order, colibri_ctx::Bigram2::Keep; csrc/bigram2.hpp
bi2_keep_kernel). bi2_emit_kernel, bi2_head_reduce_kernel, bi2_levelB_kernel and bi2_binoff_kernel read the class ids, the order-1 survivor bitmap and the plan
alone, so a run on the same upload with the same survivors starts at the count kernels, from the records, offsets, state and head lists an earlier run left.
Nothing of this may show in a model: every run here is compared with the oracle (patterns and counts, every reference list of an indexed run, found and kept per
order, tokens and types), and the same sequence with COLIBRI_BI2_KEEP=0 (read at every train(): every run partitions again) must report the same figures.
What tells a reused run from a full one: the launches of the emit2 profile class (profile=1) — none after a reused run.
What must not be reused: another threshold, another upload (either entry point, the same bytes included), whatever follows a run that failed or was repeated on
the retry ladder, a sliced order, a changed knob of the emit stage; what must not mix: two contexts alive at once."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (mintokens, maxlength, kind): one threshold; plain to 5, to 3, indexed, indexed + skipgrams, exhaustive skipgrams, plain to 5 again
RUNS = [(2, 5, {}), (2, 3, {}), (2, 4, dict(indexed=True)), (2, 4, dict(indexed=True, doskipgrams=True)), (2, 4, dict(doskipgrams_exhaustive=True)), (2, 5, {})]
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


def train_and_compare(ctx, payload, thr, maxlength, kind, sliced=False):
    """-> (the run's figures, whether order 2's partition was reused); the model is the oracle's, and order 2 ran on the second-generation engine"""
    from colibri_amd import capi
    want = _want(payload, thr, maxlength, kind)
    st = ctx.train(mintokens=thr, maxlength=maxlength, profile=1, **{k: int(v) for k, v in kind.items()})
    got, refs = ctx.export_dict()
    assert got == want.counts, (thr, maxlength, kind, len(got), len(want.counts))
    if kind.get("indexed"):
        assert refs == want.refs, (thr, maxlength, kind)
    assert (st.totaltokens, st.totaltypes) == (want.tokens, want.types), (thr, maxlength, kind)
    for n in range(1, maxlength + 1):
        assert (st.found[n], st.kept[n]) == (want.stats[n][0], want.stats[n][2]), (thr, maxlength, kind, n)
    assert ctx.last_mode() == 2 and st.path & capi.PATH_BI2 and (st.fallback_reason, st.retries) == (0, 0), (ctx.last_mode(True), st.path, st.fallback_reason, st.retries)
    assert sliced or maxlength < 3 or st.path & capi.PATH_CHAIN, st.path
    assert ctx.kernel_time(capi.K_COUNT2)[1] >= 1, "order 2's count kernels run in every run"
    return _figures(st, maxlength), ctx.kernel_time(capi.K_EMIT2)[1] == 0


def run_sequence(ctx, payload, runs, sliced=False):
    out = [train_and_compare(ctx, payload, thr, maxlength, kind, sliced) for thr, maxlength, kind in runs]
    return [f for f, _ in out], [r for _, r in out]


def corpus(name):
    from colibri_amd import synth
    if name == "zipf":  # records outside the 64 x 64 head, several B bins
        return synth.zipf_corpus(60_000, 30_000, 41, header=False)
    return synth.zipf_corpus(60_000, 30_000, 42, phrases=True, header=False)  # head pairs survive, orders 3-5 are not empty: the kept head lists after later orders have run


@pytest.fixture(scope="module")
def corpus_a():
    return corpus("zipf")


@pytest.fixture(scope="module")
def corpus_p():
    return corpus("phrases")


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


@pytest.mark.parametrize("which", ["zipf", "phrases"])
def test_runs_in_a_row_with_one_threshold(which, monkeypatch):
    """from the second run on each run is reused; models, figures and order2_records are those of the same runs with every partition repeated"""
    from colibri_amd import capi
    payload = corpus(which)
    figures, records = {}, {}
    for keep in ("1", "0"):
        monkeypatch.setenv("COLIBRI_BI2_KEEP", keep)
        with capi.Context(0) as ctx:
            ctx.upload(payload)
            figures[keep], reused = run_sequence(ctx, payload, RUNS)
            records[keep] = ctx.order2_records()  # (after the last, plain run)
        assert reused == ([False] + [True] * (len(RUNS) - 1) if keep == "1" else [False] * len(RUNS)), (keep, reused)
    assert figures["1"] == figures["0"] and records["1"] == records["0"]
    if which == "phrases":
        assert all(f[-1][2] > 0 for f in (figures["1"][0], figures["1"][-1])), "the phrase corpus keeps 5-grams: orders 3-5 ran between the reused runs"


def _with_and_without(monkeypatch, body, expect):
    """body() -> (figures, reused flags) of one sequence on contexts of its own: with the kept partition the flags are `expect`, with COLIBRI_BI2_KEEP=0 no run is
    reused, and both report the same figures"""
    figures = {}
    for keep in ("1", "0"):
        monkeypatch.setenv("COLIBRI_BI2_KEEP", keep)
        figures[keep], reused = body()
        assert reused == (expect if keep == "1" else [False] * len(expect)), (keep, reused)
    assert figures["1"] == figures["0"]
    return figures["1"]


def test_threshold_changes_are_not_reused(corpus_p, monkeypatch):
    from colibri_amd import capi

    def body():
        with capi.Context(0) as ctx:
            ctx.upload(corpus_p)
            return run_sequence(ctx, corpus_p, [(2, 4, {}), (5, 4, {}), (2, 4, {}), (2, 4, {}), (5, 4, dict(indexed=True)), (5, 3, {})])

    figures = _with_and_without(monkeypatch, body, [False, False, False, True, False, True])
    assert figures[0] == figures[2] == figures[3]


@pytest.mark.parametrize("device", [False, True], ids=["upload", "upload_device"])
def test_an_upload_drops_the_kept_partition(corpus_a, corpus_p, monkeypatch, device):
    """another corpus of the same length, then the same bytes again: each upload is partitioned anew"""
    from colibri_amd import capi

    def body():
        figures, reused = [], []
        with capi.Context(0) as ctx:
            for payload in (corpus_a, corpus_p, corpus_p):
                keep = _upload(ctx, payload, device)
                f, r = run_sequence(ctx, payload, [(2, 4, {}), (2, 4, {})])
                figures, reused = figures + f, reused + r
                del keep
        return figures, reused

    _with_and_without(monkeypatch, body, [False, True] * 3)


def test_a_failed_and_a_repeated_run_between_good_ones(monkeypatch):
    """A train() that is refused, and one whose first attempt runs out of result room (st->overflow: duplicated text keeps more patterns than the buffers start with)
    and is repeated on the retry ladder: neither leaves anything valid behind, and the runs around them are their oracles'. The good runs (plain, MAXLENGTH 3) and
    the repeated one (plain, MAXLENGTH 12) are chained runs that want the lists: one key, so only the repeat itself keeps the run after it from being reused."""
    from colibri_amd import capi, synth
    L, nsent = 12, 1500
    sent = np.random.default_rng(11).permutation(np.arange(6, 6 + L * nsent, dtype=np.uint32)).reshape(nsent, L)
    sym = np.concatenate([np.concatenate([sent, sent], axis=0), np.zeros((2 * nsent, 1), dtype=np.uint32)], axis=1).reshape(-1)
    dup = synth.encode_v2(sym).tobytes()

    def body():
        figures, reused = [], []

        def good():
            f, r = train_and_compare(ctx, dup, 2, 3, {})
            figures.append(f)
            reused.append(r)

        with capi.Context(0) as ctx:
            ctx.upload(dup)
            good()
            good()
            with pytest.raises(capi.ColibriError):
                ctx.train(mintokens=2, maxlength=3, minlength=2)
            good()  # (not reused: the refused run left nothing valid)
            good()
            want = _want(dup, 2, L, {})
            st = ctx.train(mintokens=2, maxlength=L, profile=1)  # (its first attempt finds a kept partition of its own key)
            assert ctx.export_dict()[0] == want.counts
            assert st.fallback_reason == capi.FALLBACK_RESULTS and st.retries >= 1, "the run was meant to be repeated with more room"
            assert ctx.kernel_time(capi.K_EMIT2)[1] >= 1, "a repeated attempt partitions again"
            figures.append(_figures(st, L))
            good()  # (the same key as the repeated run's: not reused only because a repeated run leaves nothing valid)
            good()
            want = _want(dup, 2, 3, dict(indexed=True))
            ctx.train(mintokens=2, maxlength=3, indexed=1, profile=1)
            assert ctx.export_dict() == (want.counts, want.refs)
        return figures, reused

    figures = _with_and_without(monkeypatch, body, [False, True, False, True, False, True])
    assert figures[0] == figures[1] == figures[2] == figures[3] == figures[5] == figures[6]


def test_two_contexts_alive_at_once(corpus_a, corpus_p, monkeypatch):
    from colibri_amd import capi

    def body():
        figures, reused = [], []

        def run(ctx, payload, thr, kind):
            f, r = train_and_compare(ctx, payload, thr, 4, kind)
            figures.append(f)
            reused.append(r)

        with capi.Context(0) as c1, capi.Context(0) as c2:
            c1.upload(corpus_a)
            c2.upload(corpus_p)
            for thr, kind in ((2, {}), (2, dict(indexed=True)), (5, {})):
                run(c1, corpus_a, thr, kind)
                run(c2, corpus_p, thr, kind)
            c1.upload(corpus_p)  # one context changes its corpus, the other keeps its partition
            run(c1, corpus_p, 5, {})
            run(c2, corpus_p, 5, {})
        return figures, reused

    _with_and_without(monkeypatch, body, [False, False, True, True, False, False, False, True])


def test_a_changed_knob_of_the_emit_stage_is_not_reused(corpus_a, monkeypatch):
    """COLIBRI_SLICED_EMIT_OFF is read by bigram2_order at every run, so its value is part of the key"""
    from colibri_amd import capi

    def body():
        monkeypatch.delenv("COLIBRI_SLICED_EMIT_OFF", raising=False)
        with capi.Context(0) as ctx:
            ctx.upload(corpus_a)
            figures, reused = run_sequence(ctx, corpus_a, [(2, 4, {}), (2, 4, {})])
            monkeypatch.setenv("COLIBRI_SLICED_EMIT_OFF", "1")
            f, r = run_sequence(ctx, corpus_a, [(2, 4, {}), (2, 4, {})])
            figures, reused = figures + f, reused + r
            monkeypatch.delenv("COLIBRI_SLICED_EMIT_OFF")
            f, r = run_sequence(ctx, corpus_a, [(2, 4, {})])
        return figures + f, reused + r

    _with_and_without(monkeypatch, body, [False, True, False, True, False])


def _worker(mode, **env):
    e = dict(os.environ, **env)
    e.pop("COLIBRI_BI2_KEEP", None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "order2_keep_worker.py"), mode], capture_output=True, text=True, env=e, timeout=300)
    assert p.returncode == 0 and "KEEP_OK" in p.stdout, p.stdout[-2000:] + p.stderr[-3000:]


def test_the_wide_form_is_reused():
    """eight sub-regions and 2048-slot tables in the orders >= 3 (COLIBRI_FORCE_WIDE_CHAIN is read once per process: a child process)"""
    _worker("wide", COLIBRI_FORCE_WIDE_CHAIN="1")


def test_a_sliced_order_is_not_kept():
    """order 2 in passes over key slices (COLIBRI_SLICE_POSITIONS is read once per process: a child process)"""
    _worker("sliced", COLIBRI_SLICE_POSITIONS="30000")
