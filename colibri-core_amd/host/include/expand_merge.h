// expand_merge.h — what a seeded device run (colibri_set_seed + colibri_train + colibri_seed_fetch) does to the host's model: train() on a loaded model
// with continued = false (patternmodel.h, train_expand). No dependency on the model classes: tests/expand_merge_check.cpp drives it on plain containers.
#ifndef COLIBRI_AMD_EXPAND_MERGE_H
#define COLIBRI_AMD_EXPAND_MERGE_H

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <vector>

namespace colibri_host {

constexpr uint32_t kNoSeedRow = 0xFFFFFFFFu;  // colibri_seed_fetch: no result row carries the seed

struct ExpandMergeCounts {
    size_t merged = 0, created = 0, erased = 0;  // loaded patterns that took a row's value, patterns inserted, loaded patterns erased
};

/** seeds[p]: the loaded pattern the p-th seed key was taken from (an iterator of `data`); row_of_seed[p] / kept[p]: colibri_seed_fetch's answer; nrows: rows
 *  of the run's result. apply(seeds[p], row): the loaded pattern takes the row's value — the count replaced by the row's sum, the row's references joined to
 *  its own; insert(row): a pattern the run created enters `data`. The seeds that do not stay are erased. A row that two seeds claim, a row beyond the result
 *  or a seed that has a row and does not stay is a broken answer: std::logic_error, `data` untouched. */
template <class Map, class Apply, class Insert>
ExpandMergeCounts expand_merge(Map& data, const std::vector<typename Map::iterator>& seeds, const std::vector<uint32_t>& row_of_seed, const std::vector<uint8_t>& kept, size_t nrows,
                               Apply apply, Insert insert) {
    if (row_of_seed.size() != seeds.size() || kept.size() != seeds.size()) throw std::logic_error("expand_merge: one row and one flag per seed");
    std::vector<uint8_t> claimed(nrows, 0);
    for (size_t p = 0; p < seeds.size(); ++p) {
        const uint32_t r = row_of_seed[p];
        if (r == kNoSeedRow) continue;
        if (r >= nrows) throw std::logic_error("expand_merge: a seed's row lies beyond the result");
        if (claimed[r]) throw std::logic_error("expand_merge: two seeds claim one row");
        if (!kept[p]) throw std::logic_error("expand_merge: a seed has a row and does not stay");
        claimed[r] = 1;
    }
    ExpandMergeCounts n;
    for (size_t p = 0; p < seeds.size(); ++p) {
        if (row_of_seed[p] != kNoSeedRow) {
            apply(seeds[p], (size_t)row_of_seed[p]);
            ++n.merged;
        } else if (!kept[p]) {
            data.erase(seeds[p]);
            ++n.erased;
        }
    }
    for (size_t r = 0; r < nrows; ++r)
        if (!claimed[r]) {
            insert(r);
            ++n.created;
        }
    return n;
}

/** an indexed pattern's references after the run: the loaded ones and the corpus', in ascending order, duplicates kept — the reference sorts every list when a
 *  train() ends (IndexedPatternModel::posttrain), so references whose sentence numbers overlap the loaded ones interleave */
template <class Ref, class It>
void expand_join_refs(std::vector<Ref>& loaded, It first, It last) {
    loaded.insert(loaded.end(), first, last);
    std::sort(loaded.begin(), loaded.end());
}

}  // namespace colibri_host

#endif
