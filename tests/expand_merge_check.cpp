// expand_merge_check.cpp — host/include/expand_merge.h on hand-made inputs, compiled with -fsanitize=address,undefined and run by tests/test_expand.py
// (test_expand_merge_under_the_sanitizers).
// Prints one line "checked <n> mismatches <m>"; exit status 1 when any case differs.
#include <cstdint>
#include <cstdio>
#include <map>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "expand_merge.h"

using colibri_host::expand_merge;
using colibri_host::ExpandMergeCounts;
using colibri_host::kNoSeedRow;

typedef std::pair<uint32_t, uint16_t> Ref;
static int checked = 0, mismatches = 0;
static void expect(bool ok, const char* what) {
    ++checked;
    if (!ok) {
        ++mismatches;
        fprintf(stderr, "MISMATCH: %s\n", what);
    }
}

// the seeds in the order of `keys`: iterators into the map, as train_expand takes them
template <class Map>
static std::vector<typename Map::iterator> seeds_of(Map& m, const std::vector<std::string>& keys) {
    std::vector<typename Map::iterator> v;
    for (const std::string& k : keys) v.push_back(m.find(k));
    return v;
}

template <class Map>
static void counts_case() {
    // loaded: a 5, b 1, c 1, d 7, e 1 (a two-token key), f 3. The run's rows: 0 = b with 1 + 1, 1 = a new key "x" 2, 2 = a with 5 + 4, 3 = a new key "y" 3.
    // c does not occur and goes (1 < 2); d does not occur and stays; e lies above the stop order and stays; f occurred once at a pruned order: 3 + 1, row 4.
    Map                      m{{"a", 5}, {"b", 1}, {"c", 1}, {"d", 7}, {"e e", 1}, {"f", 3}};
    std::vector<std::string> keys{"a", "b", "c", "d", "e e", "f"};
    std::vector<std::string> rowkey{"b", "x", "a", "y", "f"};
    std::vector<uint32_t>    rowcount{2, 2, 9, 3, 4};
    std::vector<uint32_t>    row{2, 0, kNoSeedRow, kNoSeedRow, kNoSeedRow, 4};
    std::vector<uint8_t>     kept{1, 1, 0, 1, 1, 1};
    auto                     its = seeds_of(m, keys);
    const ExpandMergeCounts  n   = expand_merge(
        m, its, row, kept, rowkey.size(), [&](typename Map::iterator it, size_t r) { it->second = rowcount[r]; }, [&](size_t r) { m[rowkey[r]] = rowcount[r]; });
    expect(n.merged == 3 && n.created == 2 && n.erased == 1, "counts: merged / created / erased");
    const Map want{{"a", 9}, {"b", 2}, {"d", 7}, {"e e", 1}, {"f", 4}, {"x", 2}, {"y", 3}};
    expect(m == want, "counts: the merged model");
}

static void refs_case() {
    // loaded references 1:6 3:7; the corpus numbered from 1 again gives 1:6 2:0: the lists interleave, duplicates kept
    std::map<std::string, std::vector<Ref>> m{{"a", {{1, 6}, {3, 7}}}, {"b", {{9, 9}}}, {"gone", {{4, 4}}}};
    std::vector<std::string>                keys{"a", "b", "gone"};
    std::vector<std::vector<Ref>>           rowrefs{{{5, 1}, {5, 2}}, {{1, 6}, {2, 0}}};  // row 0: a new key, row 1: a
    std::vector<std::string>                rowkey{"n", "a"};
    std::vector<uint32_t>                   row{1, kNoSeedRow, kNoSeedRow};
    std::vector<uint8_t>                    kept{1, 1, 0};
    auto                                    its = seeds_of(m, keys);
    expand_merge(
        m, its, row, kept, 2, [&](std::map<std::string, std::vector<Ref>>::iterator it, size_t r) { colibri_host::expand_join_refs(it->second, rowrefs[r].begin(), rowrefs[r].end()); },
        [&](size_t r) { m[rowkey[r]] = rowrefs[r]; });
    const std::map<std::string, std::vector<Ref>> want{{"a", {{1, 6}, {1, 6}, {2, 0}, {3, 7}}}, {"b", {{9, 9}}}, {"n", {{5, 1}, {5, 2}}}};
    expect(m == want, "references: joined in ascending order, duplicates kept");
}

static void empty_cases() {
    std::map<std::string, uint32_t> m{{"a", 2}};
    auto                            its = seeds_of(m, {"a"});
    // an empty result (an empty corpus): every seed stays as it is
    ExpandMergeCounts n = expand_merge(m, its, {kNoSeedRow}, {1}, 0, [&](std::map<std::string, uint32_t>::iterator, size_t) { expect(false, "empty result: nothing to apply"); },
                                       [&](size_t) { expect(false, "empty result: nothing to insert"); });
    expect(n.merged == 0 && n.created == 0 && n.erased == 0 && m.size() == 1 && m["a"] == 2, "empty result");
    // no seeds at all: every row is created
    std::map<std::string, uint32_t>                        e;
    std::vector<std::map<std::string, uint32_t>::iterator> none;
    n = expand_merge(e, none, {}, {}, 3, [&](std::map<std::string, uint32_t>::iterator, size_t) {}, [&](size_t r) { e[std::string(1, (char)('p' + r))] = (uint32_t)r + 2; });
    expect(n.created == 3 && e.size() == 3 && e["r"] == 4, "no seeds");
}

static void broken_answers() {
    const std::vector<std::vector<uint32_t>> rows{{0, 0}, {5, kNoSeedRow}, {0, kNoSeedRow}};
    const std::vector<std::vector<uint8_t>>  kepts{{1, 1}, {1, 1}, {0, 1}};
    const char* const                        what[3] = {"two seeds claim one row", "a row beyond the result", "a seed with a row that does not stay"};
    for (int k = 0; k < 3; ++k) {
        std::map<std::string, uint32_t> m{{"a", 2}, {"b", 3}};
        auto                            its    = seeds_of(m, {"a", "b"});
        bool                            thrown = false;
        try {
            expand_merge(m, its, rows[k], kepts[k], 2, [&](std::map<std::string, uint32_t>::iterator it, size_t) { it->second = 0; }, [&](size_t) { m["z"] = 0; });
        } catch (const std::logic_error&) {
            thrown = true;
        }
        expect(thrown && m == (std::map<std::string, uint32_t>{{"a", 2}, {"b", 3}}), what[k]);
    }
}

int main() {
    counts_case<std::map<std::string, uint32_t>>();
    counts_case<std::unordered_map<std::string, uint32_t>>();
    refs_case();
    empty_cases();
    broken_answers();
    printf("checked %d mismatches %d\n", checked, mismatches);
    return mismatches ? 1 : 0;
}
