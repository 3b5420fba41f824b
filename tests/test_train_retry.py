"""The retry ladder of colibri_train (colibri-core_amd/csrc/train_retry.hpp), walked on the CPU: which attempt follows which event, what colibri_stats will say.

The header is plain C++ (nothing of HIP, nothing of the context), so a stand-alone program (tests/train_retry_walk.cpp) is built against it with g++ alone and fed
event sequences; what it prints after each step is compared with the sequences written out here — the ladder as the training driver had it spread over its loops
before it became one function (DESIGN.md has the table)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REGION, BIN, IDS, ORDER2, SPLIT, CHAIN, RESULTS, PAIRS, LDS_ORDER = 1, 2, 3, 4, 8, 16, 32, 64, 128  # COLIBRI_FALLBACK_* (include/colibri_hip.h; test_abi.py pins them)


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("train_retry") / "train_retry_walk")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "colibri-core_amd", "csrc"), os.path.join(ROOT, "tests", "train_retry_walk.cpp"), "-o", exe],
                   check=True, timeout=120)

    def run(events, table_mode=0, split_exact=0, big=0):
        p = subprocess.run([exe, str(table_mode), str(split_exact), str(big)] + events.split(), capture_output=True, text=True, timeout=30)
        assert p.returncode == 0, p.stderr
        return p.stdout.splitlines()
    return run


def step(verdict, reason=0, first=0, retries=0, table=0, b2off=0, chainoff=0, small=0, split=0):
    return f"{verdict} reason={reason} first={first} retries={retries} table={table} b2off={b2off} chainoff={chainoff} small={small} split={split}"


def repeat(reason, **kw):
    kw.setdefault("first", reason)
    kw.setdefault("retries", 1)
    return step("repeat", reason, **kw)


SINGLE = [
    # the plain loop
    ("plain:0", [step("goon")]),
    ("plain:1", [repeat(REGION, table=1)]),
    ("plain:2", [repeat(BIN, table=1)]),
    ("plain:3", [repeat(IDS, table=1)]),
    ("plain:4", [repeat(ORDER2, b2off=1)]),
    ("plain:8", [repeat(SPLIT, split=1)]),
    ("plain:16", [repeat(CHAIN, chainoff=1)]),
    # the enqueued id-keeping loop: no split case (8 is a bin overflow there)
    ("enq:0", [step("goon")]),
    ("enq:1", [repeat(REGION, table=1)]),
    ("enq:2", [repeat(BIN, table=1)]),
    ("enq:3", [repeat(IDS, table=1)]),
    ("enq:4", [repeat(ORDER2, b2off=1)]),
    ("enq:8", [repeat(BIN, table=1)]),
    ("enq:16", [repeat(CHAIN, chainoff=1)]),
    # the per-pass loop: order 2 only under bi2_synced, the table only for a run on the radix path
    ("pass:0:bi2:radix", [step("goon")]),
    ("pass:1:bi2:radix", [repeat(REGION, table=1)]),
    ("pass:2:bi2:radix", [repeat(BIN, table=1)]),
    ("pass:3:bi2:radix", [repeat(IDS, table=1)]),
    ("pass:4:bi2:radix", [repeat(ORDER2, b2off=1)]),
    ("pass:8:bi2:radix", [repeat(BIN, table=1)]),
    ("pass:16:bi2:radix", [repeat(BIN, table=1)]),
    ("pass:4:radix", [repeat(BIN, table=1)]),
    ("pass:4:bi2", [repeat(ORDER2, b2off=1)]),
    ("pass:2:bi2", [step("goon")]),
    ("pass:2", [step("goon")]),
    ("pass:4", [step("goon")]),
    # the other events
    ("totable:1", [repeat(REGION, table=1)]),
    ("totable:2", [repeat(BIN, table=1)]),
    ("totable:0", [repeat(BIN, table=1)]),
    ("pairs", [repeat(PAIRS)]),
    ("ranks", [repeat(LDS_ORDER)]),
    ("results", [repeat(RESULTS)]),
]


@pytest.mark.parametrize("events,want", SINGLE, ids=[e for e, _ in SINGLE])
def test_every_single_event(walk, events, want):
    assert walk(events) == want


def test_split_overflow_with_the_exact_split_already_on(walk):
    """overflow 8 is "any other value" then: the table — or, where table_mode = 2 forbids it, the failure"""
    assert walk("plain:8", split_exact=1) == [repeat(BIN, table=1, split=1)]
    assert walk("plain:8 plain:8") == [repeat(SPLIT, split=1), repeat(BIN, first=SPLIT, retries=2, table=1, split=1)]
    assert walk("plain:8", table_mode=2, split_exact=1) == [step("fail", split=1)]
    assert walk("enq:8", split_exact=1) == [repeat(BIN, table=1, split=1)]


@pytest.mark.parametrize("loop", ["plain", "enq", "pass"])
def test_order2_overflow_with_and_without_small_passes(walk, loop):
    ev = f"{loop}:4" + (":bi2:radix" if loop == "pass" else "")
    assert walk(ev) == [repeat(ORDER2, b2off=1)]
    assert walk(ev, big=1) == [repeat(ORDER2, small=1)]
    # a second one after small passes: those stay, and the second-generation order 2 goes
    assert walk(f"{ev} {ev}", big=1) == [repeat(ORDER2, small=1), repeat(ORDER2, retries=2, small=1, b2off=1)]


def test_flags_accumulate_and_the_first_reason_stays(walk):
    assert walk("plain:16 plain:4 plain:2") == [
        repeat(CHAIN, chainoff=1),
        repeat(ORDER2, first=CHAIN, retries=2, chainoff=1, b2off=1),
        repeat(BIN, first=CHAIN, retries=3, chainoff=1, b2off=1, table=1),
    ]
    assert walk("enq:16 enq:4 enq:2") == [
        repeat(CHAIN, chainoff=1),
        repeat(ORDER2, first=CHAIN, retries=2, chainoff=1, b2off=1),
        repeat(BIN, first=CHAIN, retries=3, chainoff=1, b2off=1, table=1),
    ]


@pytest.mark.parametrize("value", [1, 2, 3, 5])
def test_table_mode_2_fails_instead_of_repeating_on_the_table(walk, value):
    assert walk(f"plain:{value}", table_mode=2) == [step("fail")]


def test_table_mode_2_keeps_the_repeats_that_stay_on_the_radix_path(walk):
    assert walk("plain:16 plain:4 plain:8 plain:2", table_mode=2) == [
        repeat(CHAIN, chainoff=1),
        repeat(ORDER2, first=CHAIN, retries=2, chainoff=1, b2off=1),
        repeat(SPLIT, first=CHAIN, retries=3, chainoff=1, b2off=1, split=1),
        step("fail", first=CHAIN, retries=3, chainoff=1, b2off=1, split=1),
    ]


def test_a_forced_table_stays_forced_through_pairs_and_ranks(walk):
    assert walk("enq:2 pairs ranks") == [
        repeat(BIN, table=1),
        repeat(PAIRS, first=BIN, retries=2, table=1),
        repeat(LDS_ORDER, first=BIN, retries=3, table=1),
    ]
    assert walk("pass:4:bi2:radix pairs") == [repeat(ORDER2, b2off=1), repeat(PAIRS, first=ORDER2, retries=2, b2off=1)]


def test_a_results_repeat_starts_clean(walk):
    assert walk("plain:16 results") == [repeat(CHAIN, chainoff=1), repeat(RESULTS, first=CHAIN, retries=2)]
    assert walk("enq:2 results results", big=1) == [repeat(BIN, table=1), repeat(RESULTS, first=BIN, retries=2), repeat(RESULTS, first=BIN, retries=3)]
    # ... but the exact split is the corpus', not the attempt's
    assert walk("plain:8 results plain:8") == [repeat(SPLIT, split=1), repeat(RESULTS, first=SPLIT, retries=2, split=1), repeat(BIN, first=SPLIT, retries=3, table=1, split=1)]
