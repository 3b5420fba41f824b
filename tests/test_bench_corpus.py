"""CPU tests: bench.py generates the timed corpus in chunks on worker processes (bench.corpus_chunk); joined in order, the chunks must be the bytes of
colibri_amd.synth.zipf_corpus, which the full-size fixtures and the suite's corpora come from."""
import pytest

import bench
from colibri_amd import synth


@pytest.mark.parametrize("tokens,vocab,seed,chunk", [
    (3_000, 50_000, 44, 1),           # a chunk per token: every sentence end falls on a chunk border
    (10_007, 200_000, 45, 7),         # borders inside sentences; 1-3-byte varints
    (100_000, 1_000_000, 44, 4096),   # the bench distribution
    (100_000, 1_000_000, 46, 100_000),  # one chunk
    (100_000, 1_000_000, 47, 1 << 23),  # the bench's own chunk size: one chunk
])
def test_joined_chunks_are_the_zipf_corpus(monkeypatch, tokens, vocab, seed, chunk):
    monkeypatch.setattr(bench, "GEN_CHUNK", chunk)
    got = b"".join(bench.corpus_chunk(s) for s in bench.corpus_chunks(tokens, vocab, seed))
    assert got == synth.zipf_corpus(tokens, vocab, seed, header=False)
