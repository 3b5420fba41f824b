// skipgram_merge_check — host/include/skipgram_merge.h on its own, built with the sanitizers by tests/test_modelskip.py: erase and insert on flat
// arrays and on a map, an answer with a bad offset refused with the model untouched, an empty answer.
#include <cstdio>
#include <map>
#include <string>
#include <utility>

#include "skipgram_merge.h"

using namespace colibri_host;

namespace {
int failures = 0;
#define CHECK(cond)                                                    \
    do {                                                               \
        if (!(cond)) {                                                 \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                \
        }                                                              \
    } while (0)

typedef std::vector<std::pair<uint32_t, uint16_t>> Refs;
typedef std::map<std::string, Refs>                Model;

struct Flat {
    std::vector<uint64_t>      key_off{0}, ref_off{0};
    std::vector<unsigned char> key_bytes;
    std::vector<uint32_t>      counts, ref_sentence;
    std::vector<uint16_t>      ref_token;
    std::vector<std::string>   order;
    void add(const std::string& key, const Refs& refs) {
        key_bytes.insert(key_bytes.end(), key.begin(), key.end());
        key_off.push_back(key_bytes.size());
        for (const auto& r : refs) {
            ref_sentence.push_back(r.first);
            ref_token.push_back(r.second);
        }
        ref_off.push_back(ref_sentence.size());
        counts.push_back((uint32_t)refs.size());
        order.push_back(key);
    }
    void slack() {  // one element behind the bytes and the references, as the exports leave them
        key_bytes.push_back(0);
        ref_sentence.push_back(0);
        ref_token.push_back(0);
    }
    Model model() const {
        Model m;
        for (size_t j = 0; j < counts.size(); ++j) {
            Refs r;
            for (uint64_t k = ref_off[j]; k < ref_off[j + 1]; ++k) r.push_back({ref_sentence[k], ref_token[k]});
            CHECK(r.size() == counts[j]);
            m[std::string(key_bytes.begin() + key_off[j], key_bytes.begin() + key_off[j + 1])] = r;
        }
        return m;
    }
};

Flat five() {
    Flat f;
    f.add("\x06", {{1, 0}, {2, 3}});
    f.add("\x06\x07\x08", {{1, 0}});
    f.add("\x07", {{1, 1}, {5, 5}, {9, 0}});
    f.add("\x06\x89\x01\x08", {{4, 2}, {4, 7}});
    f.add("\x08", {});
    f.slack();
    return f;
}
SkipgramAnswer answer(size_t np) {
    SkipgramAnswer a;
    Flat           s;
    s.add("\x06\x03\x08", {{1, 0}, {4, 2}, {4, 7}});
    s.add("\x06\x03\x03\x09", {{7, 7}});
    a.key_off = s.key_off, a.key_bytes = s.key_bytes, a.counts = s.counts, a.ref_off = s.ref_off, a.ref_sentence = s.ref_sentence, a.ref_token = s.ref_token;
    a.types = {2, 1};
    a.keep.assign(np, 1);
    return a;
}
Model expected(const Flat& f, const SkipgramAnswer& a) {
    Model m = f.model();
    for (size_t j = 0; j < a.keep.size(); ++j)
        if (!a.keep[j]) m.erase(f.order[j]);
    m["\x06\x03\x08"]     = {{1, 0}, {4, 2}, {4, 7}};
    m["\x06\x03\x03\x09"] = {{7, 7}};
    return m;
}
bool apply_to_map(Model& m, const std::vector<std::string>& order, const SkipgramAnswer& a) {
    return skipgram_merge_each(
        a, order.size(), [&](size_t j) { m.erase(order[j]); },
        [&](const unsigned char* key, size_t len, const uint32_t* s, const uint16_t* t, size_t n) {
            Refs& r = m[std::string((const char*)key, len)];
            for (size_t k = 0; k < n; ++k) r.push_back({s[k], t[k]});
        });
}
}  // namespace

int main() {
    {  // erase (the first, one in the middle, the last) and insert, flat and map
        Flat           f = five();
        SkipgramAnswer a = answer(5);
        a.keep[0] = a.keep[3] = a.keep[4] = 0;
        const Model want = expected(f, a);
        Model       m    = f.model();
        CHECK(apply_to_map(m, f.order, a) && m == want);
        size_t erased = 99;
        CHECK(skipgram_merge_flat(f.key_off, f.key_bytes, f.counts, f.ref_off, f.ref_sentence, f.ref_token, a, &erased));
        CHECK(erased == 3 && f.counts.size() == 4 && f.model() == want);
        CHECK(f.key_bytes.size() == f.key_off.back() + 1 && f.ref_sentence.size() == f.ref_off.back() + 1 && f.ref_token.size() == f.ref_off.back() + 1);
    }
    {  // nothing erased; then everything
        Flat           f = five();
        SkipgramAnswer a = answer(5);
        const Model    want = expected(f, a);
        CHECK(skipgram_merge_flat(f.key_off, f.key_bytes, f.counts, f.ref_off, f.ref_sentence, f.ref_token, a) && f.model() == want && f.counts.size() == 7);
        Flat g = five();
        a.keep.assign(5, 0);
        const Model only = expected(g, a);
        Model       m    = g.model();
        CHECK(apply_to_map(m, g.order, a) && m == only && m.size() == 2);
        CHECK(skipgram_merge_flat(g.key_off, g.key_bytes, g.counts, g.ref_off, g.ref_sentence, g.ref_token, a) && g.model() == only);
    }
    {  // malformed answers: refused, the model untouched
        const Flat f0 = five();
        for (int fault = 0; fault < 7; ++fault) {
            Flat           f = five();
            SkipgramAnswer a = answer(5);
            a.keep[1] = 0;
            switch (fault) {
                case 0: a.ref_off[1] = 9; break;                   // past the references, and not the count
                case 1: a.key_off[2] = a.key_bytes.size() + 5; break;  // past the key bytes
                case 2: a.key_off[1] = 0; break;                   // an empty key
                case 3: a.keep.pop_back(); break;                  // not one per pattern
                case 4: a.counts[0] = 2; break;                    // count != list length
                case 5: a.types.pop_back(); break;
                case 6: a.ref_off[2] = 3, a.ref_off[1] = 4; break;  // descending
            }
            CHECK(skipgram_answer_fault(a, 5) != NULL);
            Model m = f.model();
            int   calls = 0;
            CHECK(!skipgram_merge_each(a, 5, [&](size_t) { ++calls; }, [&](const unsigned char*, size_t, const uint32_t*, const uint16_t*, size_t) { ++calls; }) && calls == 0);
            CHECK(!skipgram_merge_flat(f.key_off, f.key_bytes, f.counts, f.ref_off, f.ref_sentence, f.ref_token, a));
            CHECK(f.key_off == f0.key_off && f.key_bytes == f0.key_bytes && f.counts == f0.counts && f.ref_off == f0.ref_off && f.ref_sentence == f0.ref_sentence &&
                  f.ref_token == f0.ref_token);
        }
        Flat bad = five();  // arrays that are no model: left alone
        bad.ref_off.pop_back();
        const SkipgramAnswer a = answer(5);
        CHECK(!skipgram_merge_flat(bad.key_off, bad.key_bytes, bad.counts, bad.ref_off, bad.ref_sentence, bad.ref_token, a) && bad.counts.size() == 5);
    }
    {  // an empty answer: no skipgram, every pattern kept; on an empty model too
        Flat           f = five();
        SkipgramAnswer a;
        a.key_off = {0}, a.ref_off = {0};
        a.keep.assign(5, 1);
        const Model want = f.model();
        CHECK(skipgram_answer_fault(a, 5) == NULL);
        CHECK(skipgram_answer_changes_nothing(a) && !skipgram_answer_changes_nothing(answer(5)));
        a.keep[2] = 0;
        CHECK(!skipgram_answer_changes_nothing(a));
        a.keep[2] = 1;
        CHECK(skipgram_merge_flat(f.key_off, f.key_bytes, f.counts, f.ref_off, f.ref_sentence, f.ref_token, a) && f.model() == want && f.counts.size() == 5);
        Model m = want;
        CHECK(apply_to_map(m, f.order, a) && m == want);
        Flat e;
        e.slack();
        a.keep.clear();
        CHECK(skipgram_merge_flat(e.key_off, e.key_bytes, e.counts, e.ref_off, e.ref_sentence, e.ref_token, a) && e.counts.empty() && e.key_off.size() == 1);
    }
    if (failures) return 1;
    std::printf("skipgram_merge ok\n");
    return 0;
}
