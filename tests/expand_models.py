"""Expanding a loaded model on further corpus data, restated in plain Python over the bytes of a .colibri.dat payload: the reference's train() on a
NON-EMPTY model with continued = false (include/patternmodel.h:880-1270; colibri-patternmodeller -i model -f corpus -e N without -E), for MINTOKENS >= 2,
MINLENGTH = 1, no skipgrams, no constraint, no filter, the stream form. tests/test_expand.py pins it to the real reference's results
(tests/golden/expand/); tests/test_gpu_expand.py holds the device to it. A helper module like tests/bin_models.py: nothing here needs a device.

M is the model (key bytes -> count, or -> reference list), B the new corpus with its sentences numbered from `firstsentence`. For n = 1 .. MAXLENGTH:
  1. every window of n tokens inside a sentence of B is counted iff n == 1 or both its (n-1)-token sub-windows are keys of M as M stands now
     (loaded and new alike, after the previous order's prune); a key M lacks is created;
  2. found = keys created at this order; if 0 the loop BREAKS HERE, before the prune: the counts added at this order stay, nothing of it is pruned,
     higher orders are not visited, maxn is not raised;
  3. otherwise maxn = max(maxn, n), minn = min(minn, n), and at n == 1 types = len(M) — the WHOLE model at that moment;
  4. every key of n tokens below MINTOKENS (loaded + new) is erased, loaded ones included.
tokens grows by the tokens of B. An indexed model's reference lists are sorted when the run ends (IndexedPatternModel::posttrain), every one of them."""


def sentences(payload: bytes):
    """the token byte strings of every sentence of a v2 payload (no header); empty sentences are kept: they take a sentence number"""
    toks, start, out = [], 0, []
    for j, b in enumerate(payload):
        if b >= 128:
            continue
        tok = payload[start:j + 1]
        start = j + 1
        if tok == b"\x00":
            out.append(toks)
            toks = []
        else:
            toks.append(tok)
    if toks:
        out.append(toks)
    return out


def ntokens(key: bytes) -> int:
    return sum(1 for b in key if b < 128)


class Expanded:
    """counts: key -> count; refs: key -> [(sentence, token)] (indexed) or None; stop: the order that created nothing (0: none did); found[n]: keys created at
    order n; pruned[n]: keys of n tokens the order's prune erased, loaded ones that never occurred included (no entry for the order the run stopped at)"""

    def __init__(self, counts, refs, tokens, types, maxn, minn, stop, found, pruned):
        self.counts, self.refs, self.tokens, self.types, self.maxn, self.minn, self.stop, self.found, self.pruned = counts, refs, tokens, types, maxn, minn, stop, found, pruned


def train(payload: bytes, mintokens=2, maxlength=100, indexed=False, firstsentence=1):
    """a model trained from nothing: expand() of the empty model"""
    return expand({}, payload, mintokens, maxlength, indexed=indexed, firstsentence=firstsentence, tokens=0, types=0, maxn=0, minn=99)


def expand(model, payload: bytes, mintokens=2, maxlength=100, *, indexed=False, firstsentence=1, tokens=0, types=0, maxn=0, minn=99):
    """model: key -> count (unindexed) or key -> [(sentence, token)] (indexed), n-grams only; tokens / types / maxn / minn: the loaded model's"""
    thr = 2 if mintokens == -1 else mintokens
    assert thr >= 2
    M = {k: (list(v) if indexed else int(v)) for k, v in model.items()}
    sents = sentences(payload)
    tokens += sum(len(s) for s in sents)
    stop, found_n, pruned_n = 0, {}, {}
    for n in range(1, maxlength + 1):
        before = len(M)
        sentence = firstsentence - 1
        for toks in sents:
            sentence += 1
            for i in range(len(toks) - n + 1):
                if n > 1 and not (b"".join(toks[i:i + n - 1]) in M and b"".join(toks[i + 1:i + n]) in M):
                    continue
                k = b"".join(toks[i:i + n])
                if indexed:
                    M.setdefault(k, []).append((sentence, i))
                else:
                    M[k] = M.get(k, 0) + 1
        found_n[n] = len(M) - before
        if found_n[n] == 0:
            stop = n
            break
        maxn, minn = max(maxn, n), min(minn, n)
        if n == 1:
            types = len(M)
        gone = [k for k, v in M.items() if ntokens(k) == n and (len(v) if indexed else v) < thr]
        pruned_n[n] = len(gone)
        for k in gone:
            del M[k]
    if indexed:
        refs = {k: sorted(v) for k, v in M.items()}
        return Expanded({k: len(v) for k, v in refs.items()}, refs, tokens, types, maxn, minn, stop, found_n, pruned_n)
    return Expanded(M, None, tokens, types, maxn, minn, stop, found_n, pruned_n)


def naive_sum(a: dict, b: dict) -> dict:
    """what adding two separately trained models gives: the wrong answer the fixtures are chosen to expose"""
    out = dict(a)
    for k, v in b.items():
        out[k] = out.get(k, 0) + v
    return out


def parse_golden(text: str):
    """a dump of the scratch driver: '#tokens', '#types', '#patterns', '#maxn', '#minn', then <hex key>\\t<count>[\\t<sentence>:<token> ...]"""
    head, counts, refs = {}, {}, {}
    for ln in text.splitlines():
        if ln.startswith("#"):
            name, value = ln[1:].split()
            head[name] = int(value)
            continue
        parts = ln.split("\t")
        k = bytes.fromhex(parts[0])
        counts[k] = int(parts[1])
        if len(parts) > 2:
            refs[k] = [tuple(int(x) for x in r.split(":")) for r in parts[2].split(" ") if r]
    assert len(counts) == head["patterns"]
    return head, counts, (refs if refs else None)
