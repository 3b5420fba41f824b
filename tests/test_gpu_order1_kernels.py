"""GPU: the order-1 kernels (csrc/kernels.hpp: uni_onepass_kernel, its epilogue, uni_finish_kernel) at the sizes where they change path. Class arrays built by hand,
MAXLENGTH 2, every model compared with the oracle (patterns and counts, found and kept per order, tokens and types):
positions of 1, 5 000, 8 191, 8 192, 8 193 and 3 x 8 192 + 2 (a tile is 8 192 positions: every remainder of a tile's loads); 8 191, 8 192, 8 193 and 70 001 classes
(the LDS head ends at class 8 191; a partial group of 16 classes; a partial finish tile; more than 16 rows of 4 096 classes per tail bin); every token of one class,
below and above the head (the second fills one tail bin by itself: the overflow route, with global atomics); tail classes that all fall into one bin
((c >> 4) & 255 constant). All of it again with a room of 8 tokens per tail bin (COLIBRI_UNI_BIN_CAP, read at every train()), and every corpus trained twice: the
second run reads the counts the first one left."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TILE = 8192


def _sentences(toks, every=17):
    """class ids with a delimiter at every 17th position: len(result) == len(toks) positions"""
    sym = np.asarray(toks, dtype=np.uint32).copy()
    sym[every - 1::every] = 0
    return sym


def _mixed(npos, maxclass, seed):
    """head and tail classes, the rare ones twice at least, class `maxclass` among them"""
    rng = np.random.default_rng(seed)
    half = max(1, npos // 2)
    heavy = 6 + np.minimum(rng.pareto(0.7, size=half).astype(np.int64), maxclass - 6)
    spread = rng.integers(6, maxclass + 1, size=max(1, (npos - half + 1) // 2))
    toks = np.concatenate([heavy, spread, spread])[:npos].astype(np.uint32)
    if npos >= 40:
        toks[[2, 20]] = maxclass
    return _sentences(rng.permutation(toks)) if npos > 1 else toks[:1]


def _cases():
    out = {}
    for npos in (1, 5000, TILE - 1, TILE, TILE + 1, 3 * TILE + 2):
        out[f"npos_{npos}"] = _mixed(npos, 20000, npos)
    for nclasses in (8191, 8192, 8193, 70001):
        out[f"classes_{nclasses}"] = _mixed(30000, nclasses - 1, nclasses)
    out["one_head_class"] = _sentences(np.full(3 * TILE + 2, 100, dtype=np.uint32))
    out["one_tail_class"] = _sentences(np.full(3 * TILE + 2, 9000, dtype=np.uint32))
    rng = np.random.default_rng(77)
    one_bin = ((rng.integers(2, 17, size=40000) << 12) | (0x2A << 4) | rng.integers(0, 16, size=40000)).astype(np.uint32)
    one_bin[::3] = rng.integers(6, 200, size=one_bin[::3].size)  # (a third of the tokens in the head)
    out["one_tail_bin"] = _sentences(one_bin)
    return out


CASES = _cases()
_ORACLE = {}


def _want(name):
    import oracle
    from colibri_amd import synth
    if name not in _ORACLE:
        payload = synth.encode_v2(CASES[name]).tobytes()
        _ORACLE[name] = (payload, oracle.train(payload, 2, 2))
    return _ORACLE[name]


@pytest.mark.parametrize("bin_cap", [None, "8"], ids=["default_room", "room_of_8"])
@pytest.mark.parametrize("name", list(CASES))
def test_order1_at_its_edges(monkeypatch, name, bin_cap):
    from colibri_amd import capi
    monkeypatch.delenv("COLIBRI_UNI_CACHE", raising=False)
    if bin_cap is None:
        monkeypatch.delenv("COLIBRI_UNI_BIN_CAP", raising=False)
    else:
        monkeypatch.setenv("COLIBRI_UNI_BIN_CAP", bin_cap)
    payload, want = _want(name)
    sym = CASES[name]
    with capi.Context(0) as ctx:
        ctx.upload(payload)
        assert ctx.positions() == sym.size and ctx.corpus_info()["maxclass"] == int(sym.max())
        for rep in range(2):
            st = ctx.train(mintokens=2, maxlength=2)
            got, _ = ctx.export_dict()
            assert got == want.counts, (name, rep, len(got), len(want.counts))
            assert (st.totaltokens, st.totaltypes) == (want.tokens, want.types), (name, rep)
            assert st.admitted[1] == int(np.count_nonzero(sym)), (name, rep)
            for n in (1, 2):
                assert (st.found[n], st.kept[n]) == (want.stats[n][0], want.stats[n][2]), (name, rep, n)
