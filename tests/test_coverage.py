"""The coverage report (colibri-patternmodeller -R / -r; colibri_coverage, csrc/coverage.hpp), without a device: a restatement of the four plain
per-group values from a model's flat arrays, checked — with the quirks report() applies to them — against the text the reference prints for the
model files of tests/golden/views/; and the presence of the new entry points. test_gpu_coverage.py holds the device to this restatement."""
import os

import numpy as np
import pytest

from test_views import CASES, GOLD, VIEWS, golden

CATEGORY_NAMES = ["all", "n-gram", "skipgram", "flexgram"]


def tokens_of(key):
    """the tokens of a key as class ids: a byte under 128 closes a token, seven bits per byte, least significant first"""
    out, cur, shift = [], 0, 0
    for b in key:
        cur |= (b & 127) << shift
        shift += 7
        if b < 128:
            out.append(cur)
            cur, shift = 0, 0
    return out


def category_of(toks):
    """the first gap decides: {*} (class 3) a skipgram, {**} (class 4) a flexgram"""
    for t in toks:
        if t == 3:
            return 2
        if t == 4:
            return 3
    return 1


def coverage_groups(key_off, key_bytes, counts=None, refs=None, per_size=False):
    """(patterns, counts, types, tokens), each [category][size] with 0 = all and sizes up to the longest pattern — the plain values:
    a pattern of category c and n tokens belongs to (0, 0), (c, 0), (0, n), (c, n); a flexgram adds to patterns / counts of the all-sizes groups only;
    types = distinct class ids of the group's patterns, gap markers included; tokens = distinct (sentence, (token + i) mod 65536), i < n, over the
    references of the group's patterns — per-size groups only with per_size, all 0 without references"""
    kb, off = bytes(bytearray(np.asarray(key_bytes, dtype=np.uint8).tolist())), [int(x) for x in key_off]
    npat = len(off) - 1
    toks = [tokens_of(kb[off[j]:off[j + 1]]) for j in range(npat)]
    G = max([len(t) for t in toks], default=-1) + 1
    patterns = [[0] * G for _ in range(4)]
    occ = [[0] * G for _ in range(4)]
    types = [[set() for _ in range(G)] for _ in range(4)]
    covered = [[set() for _ in range(G)] for _ in range(4)]
    if refs is not None:
        ref_off, rs, rt = refs
        ref_off, rs, rt = [int(x) for x in ref_off], [int(x) for x in rs], [int(x) for x in rt]
    for j, t in enumerate(toks):
        c, n = category_of(t), len(t)
        count = int(counts[j]) if counts is not None else ref_off[j + 1] - ref_off[j]
        for gc in (0, c):
            for gn in (0, n):
                if not (c == 3 and gn != 0):
                    patterns[gc][gn] += 1
                    occ[gc][gn] += count
                types[gc][gn].update(t)
        if refs is not None:
            pos = {(rs[r], (rt[r] + i) & 0xFFFF) for r in range(ref_off[j], ref_off[j + 1]) for i in range(n)}
            for gc in (0, c):
                covered[gc][0] |= pos
                if per_size:
                    covered[gc][n] |= pos
    as_array = lambda rows: np.array(rows, dtype=np.uint64).reshape(4, G)
    return (as_array(patterns), as_array(occ), as_array([[len(s) for s in row] for row in types]), as_array([[len(s) for s in row] for row in covered]))


def report_text(groups, indexed, total_tokens, total_types, coverage=True):
    """what PatternModel::report() prints from the plain values (host/include/patternmodel.h): per-size token rows of an indexed model are 0, every
    group of an unindexed one gets the sum of all counts, a flexgram has no per-size row"""
    patterns, occ, types, tokens = [a.tolist() for a in groups]
    G = len(patterns[0])
    W = 15
    col = lambda v: str(v).rjust(W)
    frac = lambda v: ("%.4f" % v).rjust(W)
    out = ["", "REPORT"]
    if not indexed and coverage:
        out += ["   Warning: Model is unindexed, token coverage counts are mere maximal projections",
                "            assuming no overlap at all!!! Use an indexed model for accurate coverage counts"]
    out += ["-" * 34, " " * 26 + col("PATTERNS") + col("TOKENS") + col("COVERAGE") + col("TYPES"),
            "Total:".ljust(26) + col("-") + col(total_tokens) + col("-") + col(total_types)]
    group_tokens = lambda c, n: (tokens[c][0] if n == 0 else 0) if indexed else occ[0][0]
    if coverage:
        covered = min(group_tokens(0, 0), total_tokens)
        out += ["Uncovered:".ljust(26) + col("-") + col(total_tokens - covered) + frac((total_tokens - covered) / total_tokens) + col(total_types - types[0][0]),
                "Covered:".ljust(26) + col(patterns[0][0]) + col(covered) + frac(covered / total_tokens) + col(types[0][0])]
    out.append("")
    head = col("CATEGORY") + col("N (SIZE) ") + col("PATTERNS")
    if indexed and coverage:
        head += col("TOKENS") + col("COVERAGE")
    if coverage:
        head += col("TYPES")
    out.append(head + col("OCCURRENCES"))
    for c in range(4):
        for n in range(G):
            if not patterns[c][n]:
                continue
            row = col(CATEGORY_NAMES[c]) + col("all" if n == 0 else n) + col(patterns[c][n])
            if indexed and coverage:
                row += col(group_tokens(c, n)) + frac(group_tokens(c, n) / total_tokens)
            if coverage:
                row += col(types[c][n])
            out.append(row + col(occ[c][n]))
    return ("\n".join(out) + "\n").encode()


def load_case(case):
    """a model file of tests/golden/views/ as flat arrays: (indexed, tokens, types, key_off, key_bytes, counts, refs)"""
    from colibri_amd import digest
    mtype, tokens, types, key_off, key_bytes, counts, refs = digest.parse_model_file(os.path.join(VIEWS, f"{case}.colibri.patternmodel"))
    return mtype == 20, int(tokens), int(types), key_off, key_bytes, counts, refs


@pytest.mark.parametrize("case", list(CASES))
def test_restatement_reproduces_the_reference_reports(case):
    indexed, tokens, types, key_off, key_bytes, counts, refs = load_case(case)
    groups = coverage_groups(key_off, key_bytes, None if indexed else counts, refs)
    assert report_text(groups, indexed, tokens, types) == golden(case, "report")
    assert report_text(groups, indexed, tokens, types, coverage=False) == golden(case, "simplereport")


def test_restatement_on_a_model_written_by_hand():
    """two sentences: overlapping references cover a position once, a gap is a type and a covered position, a flexgram has no per-size patterns or
    counts, and a token index past 65535 starts again at 0"""
    keys = [b"\x05", b"\x05\x06", b"\x05\x03\x06", b"\x81\x01\x04\x05"]  # a | a b | a {*} b | <129> {**} a
    refs = [[(1, 0), (1, 1), (2, 0)], [(1, 1), (2, 0)], [(1, 0)], [(2, 65535)]]
    key_off = np.cumsum([0] + [len(k) for k in keys]).astype(np.uint64)
    ref_off = np.cumsum([0] + [len(r) for r in refs]).astype(np.uint64)
    rs = np.array([s for r in refs for s, _ in r], dtype=np.uint32)
    rt = np.array([t for r in refs for _, t in r], dtype=np.uint16)
    patterns, occ, types, tokens = coverage_groups(key_off, np.frombuffer(b"".join(keys), dtype=np.uint8), None, (ref_off, rs, rt), per_size=True)
    assert patterns.tolist() == [[4, 1, 1, 1], [2, 1, 1, 0], [1, 0, 0, 1], [1, 0, 0, 0]]
    assert occ.tolist() == [[7, 3, 2, 1], [5, 3, 2, 0], [1, 0, 0, 1], [1, 0, 0, 0]]
    assert types.tolist() == [[5, 1, 2, 5], [2, 1, 2, 0], [3, 0, 0, 3], [3, 0, 0, 3]]  # {5, 6, 3, 129, 4}
    # (1, 0..2), (2, 0..1) from the n-grams and the skipgram; the flexgram at token 65535 wraps: (2, 65535), (2, 0), (2, 1)
    assert tokens.tolist() == [[6, 3, 4, 6], [5, 3, 4, 0], [3, 0, 0, 3], [3, 0, 0, 3]]


def test_the_library_and_the_python_face_have_the_coverage_calls():
    from colibri_amd import capi
    L = capi.load()
    for name in ("colibri_coverage", "colibri_coverage_resident", "colibri_coverage_fetch", "colibri_coverage_info"):
        assert name in capi.EXPORTED and hasattr(L, name)
    for method in ("coverage", "coverage_resident", "coverage_info"):
        assert callable(getattr(capi.Context, method))
    assert capi.COV_PER_SIZE == 1 and capi.COV_NO_TOKENS == 2
