"""Every entry point that takes a pattern model takes it in two forms: host arrays in export layout, and the model the last train() left in
HBM. Both reach the device pipelines as one view (csrc/model_api.inc), so both must give every consumer the same model, and neither may write
into the context: here each consumer is called resident, loaded from export_arrays() of the same context, and resident again, and the three
results must be identical array for array."""
import numpy as np
import pytest

from conftest import small_corpora

pytestmark = pytest.mark.gpu

WORDS = {k: "w%d" % k for k in range(1, 64)}  # (an id above them prints {?})
INDEXED_ONLY = ("flexgrams", "cooc", "skipcontent", "coverage", "coverage_per_size") + tuple("relations%d" % k for k in range(6))


@pytest.fixture(scope="module")
def ctx():
    from colibri_amd import capi
    with capi.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def corpora():
    return small_corpora()


def consumers(ctx, tokens):
    """name -> (the resident call, the loaded call on export_arrays()' (key_off, key_bytes, counts, refs | None), the rows of a result)"""
    from colibri_amd import capi
    refs = lambda m: m[3] if m[3] is not None else (None, None, None)
    out = {
        "flexgrams": (ctx.flexgrams_resident, lambda m: ctx.flexgrams(m[0], m[1], *refs(m)), lambda r: len(r[2])),
        "cooc": (lambda: ctx.cooc_resident(0, capi.COOC_COUNT), lambda m: ctx.cooc(m[0], m[1], *refs(m), threshold=0, mode=capi.COOC_COUNT), lambda r: len(r[0])),
        "skipcontent": (ctx.skipcontent_resident, lambda m: ctx.skipcontent(m[0], m[1], *refs(m)), lambda r: len(r[0])),
        "coverage": (ctx.coverage_resident, lambda m: ctx.coverage(m[0], m[1], m[2], *refs(m)), lambda r: r[0].size),
        "coverage_per_size": (lambda: ctx.coverage_resident(per_size=True), lambda m: ctx.coverage(m[0], m[1], m[2], *refs(m), per_size=True), lambda r: r[0].size),
        "print_model": (lambda: ctx.print_model(WORDS, None, tokens), lambda m: ctx.print_model(WORDS, m, tokens), len),
        "histogram": (lambda: ctx.histogram(None), ctx.histogram, lambda r: len(r[0])),
        "reverse_index": (lambda: ctx.reverse_index(resident=True), lambda m: ctx.reverse_index(m[0], m[1], m[2]), lambda r: len(r[3])),
    }
    for kind in range(6):
        out["relations%d" % kind] = (lambda kind=kind: ctx.relations_resident(kind, 0), lambda m, kind=kind: ctx.relations(m[0], m[1], *refs(m), kind, 0), lambda r: len(r[0]))
    return out


def same(a, b):
    if isinstance(a, (tuple, list)):
        return isinstance(b, (tuple, list)) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)
    return type(a) is type(b) and a == b


def three_calls(ctx, tokens, names=None):
    """every consumer resident, loaded, resident: {name: (the result, its rows)}"""
    got = {}
    for name, (resident, loaded, rows) in consumers(ctx, tokens).items():
        if names is not None and name not in names:
            continue
        first = resident()
        second = loaded(ctx.export_arrays())
        third = resident()
        assert same(first, second), f"{name}: the loaded form differs from the resident form"
        assert same(first, third), f"{name}: the resident form differs after a loaded call"
        got[name] = (first, rows(first))
    return got


def train(ctx, payload, **kw):
    ctx.upload(payload)
    return ctx.train(**kw).totaltokens


def test_indexed_model_with_skipgrams(ctx, corpora):
    tokens = train(ctx, corpora["rand1"], indexed=1, doskipgrams=1, mintokens=2, maxlength=5)
    got = three_calls(ctx, tokens)
    for name in ("flexgrams", "cooc", "skipcontent", "relations0", "relations5", "print_model", "histogram", "reverse_index"):  # (n-gram and masked segments both took part)
        assert got[name][1] > 0, name


def test_multibyte_classes(ctx, corpora):
    tokens = train(ctx, corpora["multibyte"], indexed=1, mintokens=2, maxlength=3)
    key_off, key_bytes, counts, _ = ctx.export_arrays()
    assert len(key_bytes) > 2 * len(counts)  # (key bytes differ from token counts)
    got = three_calls(ctx, tokens)
    assert got["cooc"][1] > 0 and got["reverse_index"][1] > 0


def test_trained_model_of_no_patterns(ctx, corpora):
    tokens = train(ctx, corpora["one_token"], indexed=1, mintokens=2)
    assert ctx.result_sizes()[0] == 0
    for name, (_, rows) in three_calls(ctx, tokens).items():
        assert rows == 0, name


def test_unindexed_model(ctx, corpora):
    from colibri_amd import capi
    tokens = train(ctx, corpora["rand1"], indexed=0, mintokens=2, maxlength=4)
    got = three_calls(ctx, tokens, ("print_model", "histogram", "reverse_index"))
    assert all(rows > 0 for _, rows in got.values())
    for name, (resident, _, _) in consumers(ctx, tokens).items():
        if name in INDEXED_ONLY:
            with pytest.raises(capi.ColibriError) as e:
                resident()
            assert e.value.code == -6, name  # COLIBRI_ERR_STATE
    values, patterns = np.unique(ctx.export_arrays()[2], return_counts=True)
    counts, npatterns = ctx.histogram(None)
    assert counts.tolist() == values.tolist() and npatterns.tolist() == patterns.tolist()
    assert same((counts, npatterns), got["histogram"][0])


def test_nothing_writes_into_the_resident_model(ctx, corpora):
    for name, kw in (("multibyte", dict(indexed=1, mintokens=2, maxlength=3)), ("rand1", dict(indexed=0, mintokens=2, maxlength=4))):  # (a context that has held other models)
        train(ctx, corpora[name], **kw)
    tokens = train(ctx, corpora["rand1"], indexed=1, doskipgrams=1, mintokens=2, maxlength=5)
    before = ctx.export_arrays()
    three_calls(ctx, tokens)
    assert same(before, ctx.export_arrays())
