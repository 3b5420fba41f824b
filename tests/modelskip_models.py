"""The skipgrams of an indexed model that already holds its n-grams — IndexedPatternModel::trainskipgrams on a loaded model, what
colibri-patternmodeller -i model -s runs — restated plainly on dictionaries, the fixture loaders of tests/golden/modelskip/
and the flat-array forms the device entry points take. Shared by tests/test_modelskip.py (CPU) and tests/test_gpu_modelskip.py."""
import gzip
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = os.path.join(GOLDEN, "modelskip")
GAP = b"\x03"
FLEX = b"\x04"


def varint(cls):
    """class id -> its key bytes: 7 bits per byte, low bits first, the high bit on every byte but the last"""
    out = bytearray()
    while cls >= 128:
        out.append(0x80 | (cls & 0x7F))
        cls >>= 7
    out.append(cls)
    return bytes(out)


def tokens_of(key):
    """key bytes -> tuple of tokens (a token ends at its first byte < 128)"""
    out, cur = [], bytearray()
    for b in key:
        cur.append(b)
        if b < 128:
            out.append(bytes(cur))
            cur = bytearray()
    assert not cur, "key ends inside a token"
    return tuple(out)


def gap_masks(n, maxskips):
    """compute_skip_configurations(n, maxskips): bit i = token i is a gap; never at either end; at most maxskips separate gaps once n - 2 >= maxskips"""
    out = []
    for i in range(1, 1 << (n - 2)):
        mask = i << 1
        runs = sum(1 for k in range(n) if (mask >> k) & 1 and not (k and (mask >> (k - 1)) & 1))
        if n - 2 >= maxskips and runs > maxskips:
            continue
        out.append(mask)
    return out


def restate(model, mintokens=2, mintokens_skipgrams=-1, minskiptypes=2, maxlength=100, maxskips=3, trace=None):
    """model: {tuple of tokens: list of (sentence, token)}, changed in place as trainskipgrams changes it (every list it adds ascending).
    Returns (per order looked at [n, found, pruned, extra] — the last may have found nothing: the loop ended there, before any prune —,
    hasskipgrams, {skipgram: its number of source n-grams} for the kept ones). trace (a dict): "candidates" = (valid source, mask) pairs over all
    orders, "groups" = {skipgram: (count, sources)} of every skipgram found, kept or not, "invalid" = the n-grams a missing slice kept out."""
    t = 2 if mintokens == -1 else mintokens
    msk = max(mintokens_skipgrams, t)
    log, has, types = [], False, {}
    trace = {} if trace is None else trace
    trace.update(candidates=0, groups={}, invalid=[])
    for n in range(3, maxlength + 1):
        masks = gap_masks(n, maxskips) if n <= 31 else []
        new, src = {}, {}
        for k in [k for k in model if len(k) == n and GAP not in k and FLEX not in k]:
            if msk > 1 and not (k[:-1] in model and k[1:] in model):
                trace["invalid"].append(k)
                continue
            trace["candidates"] += len(masks)
            for mask in masks:
                sk = tuple(GAP if (mask >> i) & 1 else tok for i, tok in enumerate(k))
                new.setdefault(sk, []).extend(model[k])
                src[sk] = src.get(sk, 0) + 1
        if not new:
            log.append([n, 0, 0, 0])
            break
        has = True
        trace["groups"].update({sk: (len(refs), src[sk]) for sk, refs in new.items()})
        assert not any(sk in model for sk in new), "the model held skipgrams already"
        model.update({sk: sorted(refs) for sk, refs in new.items()})
        low = [k for k in model if len(k) == n and len(model[k]) < t]
        for k in low:
            del model[k]
        few = [k for k in new if k in model and minskiptypes > 1 and src[k] < minskiptypes]
        for k in few:
            del model[k]
        types.update({k: src[k] for k in new if k in model})
        log.append([n, len(new), len(low), len(few)])
    return log, has, types


def progress_lines(log):
    """the lines trainskipgrams writes to stderr unless QUIET, the unsigned 32-bit `total kept` included"""
    out = ["Finding skipgrams on the basis of extracted n-grams..."]
    for n, found, pruned, extra in log:
        out.append("Counting %d-skipgrams" % n)
        if not found:
            out.append(" None found")
            break
        line = " Found %d skipgrams...pruned %d" % (found, pruned)
        if extra:
            line += " plus %d extra skipgrams.." % extra
        out.append(line + "...total kept: %d" % ((found - pruned - extra) & 0xFFFFFFFF))
    return out


# ---- fixtures --------------------------------------------------------------------------------------------------------------------------------
def _open(path):
    return gzip.open(path, "rt") if path.endswith(".gz") else open(path)


def load_rows(path):
    """`<hex key>\\t<count>\\t<s:t ...>` rows (lines starting with # are skipped) -> {tokens: sorted [(s, t)]}"""
    if not os.path.exists(path) and os.path.exists(path + ".gz"):
        path += ".gz"
    model = {}
    with _open(path) as f:
        for line in f:
            if line.startswith("#") or not line.strip():
                continue
            p = line.rstrip("\n").split("\t")
            refs = sorted(tuple(map(int, r.split(":"))) for r in p[2].split()) if len(p) > 2 else []
            assert len(refs) == int(p[1]), (path, p[0])
            model[tokens_of(bytes.fromhex(p[0]))] = refs
    return model


def cases():
    with open(os.path.join(FIXTURES, "cases.json")) as f:
        return json.load(f)


def fixture(name):
    """(options of the case, the loaded model, the model the reserved reference left, its stderr lines)"""
    c = cases()[name]
    with open(os.path.join(FIXTURES, name + ".stderr.txt")) as f:
        err = f.read().splitlines()
    return c, load_rows(os.path.join(FIXTURES, c["loaded"])), load_rows(os.path.join(FIXTURES, c["after"])), err  # (cases that share a dump name one file)


def case_options(c):
    return dict(mintokens=c["t"], mintokens_skipgrams=c["y"], minskiptypes=c["T"], maxlength=c["l"], maxskips=3)


# the direct -s builds tests/golden/ already holds, beside the n-gram models they must come from: (i golden, is golden, options). No n-gram golden
# was recorded at MAXLENGTH 100: there the start is the is golden's own n-grams (None), which a build at one threshold leaves as they were
DIRECT = [
    ("hamlet.v2.i.l5.txt", "hamlet.v2.is.l5.txt", dict(mintokens=2, minskiptypes=2, maxlength=5)),
    ("hamlet.v2.i.l5.txt", "hamlet.v2.isT1.l5.txt", dict(mintokens=2, minskiptypes=1, maxlength=5)),
    (None, "hamlet.v2.is.l100.txt", dict(mintokens=2, minskiptypes=2, maxlength=100)),
    ("zipf20k.i.l5.txt", "zipf20k.is.l5.txt", dict(mintokens=2, minskiptypes=2, maxlength=5)),
    ("zipf20k.i.l5.txt", "zipf20k.isT1.l5.txt", dict(mintokens=2, minskiptypes=1, maxlength=5)),
    ("phrases15k.i.l5.txt", "phrases15k.is.l5.txt", dict(mintokens=2, minskiptypes=2, maxlength=5)),
    ("phrases15k.i.l5.txt", "phrases15k.isT1.l5.txt", dict(mintokens=2, minskiptypes=1, maxlength=5)),
]


def direct_pair(igold, isgold):
    """(the n-gram model to start from, the model the direct -s build left)"""
    want = load_rows(os.path.join(GOLDEN, isgold))
    start = load_rows(os.path.join(GOLDEN, igold)) if igold else {k: v for k, v in want.items() if GAP not in k}
    return start, want


# ---- flat arrays -----------------------------------------------------------------------------------------------------------------------------
def to_arrays(model, order=None):
    """{tokens: refs} -> (key_off, key_bytes, ref_off, ref_s, ref_t, keys in that order); order: the keys' order (default: sorted by bytes)"""
    keys = list(order) if order is not None else sorted(model, key=lambda k: b"".join(k))
    kb = [b"".join(k) for k in keys]
    key_off = np.zeros(len(keys) + 1, dtype=np.uint64)
    key_off[1:] = np.cumsum([len(b) for b in kb], dtype=np.uint64)
    ref_off = np.zeros(len(keys) + 1, dtype=np.uint64)
    ref_off[1:] = np.cumsum([len(model[k]) for k in keys], dtype=np.uint64)
    flat = [r for k in keys for r in model[k]]
    ref_s = np.array([r[0] for r in flat], dtype=np.uint32)
    ref_t = np.array([r[1] for r in flat], dtype=np.uint16)
    return key_off, np.frombuffer(b"".join(kb), dtype=np.uint8), ref_off, ref_s, ref_t, keys


def answer_rows(answer):
    """what Context.model_skipgrams returns -> ([(tokens, count, types, [(s, t)])] in answer order, keep as a list)"""
    so, sk, sc, sy, (sro, srs, srt), keep = answer
    kb, off, ro = sk.tobytes(), so.tolist(), sro.tolist()
    s, t = srs.tolist(), srt.tolist()
    rows = [(tokens_of(kb[off[j]:off[j + 1]]), int(sc[j]), int(sy[j]), list(zip(s[ro[j]:ro[j + 1]], t[ro[j]:ro[j + 1]]))) for j in range(len(sc))]
    return rows, keep.tolist()


def apply_answer(model, keys, answer):
    """the model after the answer is installed: the patterns whose keep byte is 0 leave, the skipgrams enter with their lists as they came"""
    rows, keep = answer_rows(answer)
    assert len(keep) == len(keys)
    out = {k: model[k] for k, flag in zip(keys, keep) if flag}
    for k, cnt, _, refs in rows:
        assert k not in out and cnt == len(refs)
        out[k] = refs
    return out
