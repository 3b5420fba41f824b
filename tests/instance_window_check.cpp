// instance_window_check.cpp — host/include/instance_window.h on hand-made corpora, compiled with -fsanitize=address,undefined and run by tests/test_instantiate.py
// (test_instance_window_under_the_sanitizers). Every payload lives in a heap block of exactly its size, so a read past it is an error of the run.
// Prints one line "checked <n> mismatches <m>"; exit status 1 when any case differs.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "instance_window.h"

using colibri_host::instance_window;
using colibri_host::InstanceWindow;

static int checked = 0, mismatches = 0;
static void expect(bool ok, const char* what) {
    ++checked;
    if (!ok) {
        ++mismatches;
        fprintf(stderr, "MISMATCH: %s\n", what);
    }
}

struct Corpus {
    std::unique_ptr<unsigned char[]> bytes;  // exactly n bytes
    size_t                           n = 0;
    std::vector<uint64_t>            start;  // every delimiter opens a sentence, empty ones included, none after the last byte
    explicit Corpus(const std::string& s) : bytes(new unsigned char[s.size() ? s.size() : 1]), n(s.size()) {
        if (n) std::memcpy(bytes.get(), s.data(), n);
        bool prevdelimiter = true, prevhigh = false;
        for (size_t i = 0; i < n; ++i) {
            if (prevdelimiter) start.push_back(i);
            prevdelimiter = !prevhigh && bytes[i] == 0;
            prevhigh      = bytes[i] >= 128;
        }
    }
    InstanceWindow at(uint32_t first, uint32_t s, uint32_t t, uint32_t len) const { return instance_window(bytes.get(), n, start.data(), start.size(), first, s, t, len); }
    bool is(const InstanceWindow& w, const std::string& want) const { return w.fits && w.bytes == want.size() && std::memcmp(bytes.get() + w.begin, want.data(), want.size()) == 0; }
};

int main() {
    // sentence 1: 5 6 7 8; sentence 2: empty; sentence 3: 300 (AC 02) 9 2^21+7 (87 80 80 01); sentence 4: 10, without a delimiter behind it
    const std::string s1("\x05\x06\x07\x08", 4), s3("\xac\x02\x09\x87\x80\x80\x01", 7);
    const Corpus      c(s1 + std::string(1, '\0') + std::string(1, '\0') + s3 + std::string(1, '\0') + "\x0a");
    expect(c.start.size() == 4 && c.start[1] == 5 && c.start[2] == 6 && c.start[3] == 14, "the sentence index");
    expect(c.is(c.at(1, 1, 0, 4), s1), "the whole first sentence");
    expect(c.is(c.at(1, 1, 0, 3), s1.substr(0, 3)), "a window at a sentence's first token");
    expect(c.is(c.at(1, 1, 1, 3), s1.substr(1)), "a window that ends at a sentence's last token");
    expect(c.is(c.at(1, 1, 3, 1), s1.substr(3)), "the last token alone");
    expect(!c.at(1, 1, 0, 5).fits && !c.at(1, 1, 2, 3).fits && !c.at(1, 1, 4, 1).fits, "a window one token too long");
    expect(!c.at(1, 1, 5, 1).fits && !c.at(1, 1, 65535, 3).fits, "a token beyond the sentence");
    expect(!c.at(1, 2, 0, 1).fits && !c.at(1, 2, 0, 3).fits && !c.at(1, 2, 1, 1).fits, "an empty sentence holds no window");
    expect(c.at(1, 2, 0, 0).fits && c.at(1, 2, 0, 0).bytes == 0, "... but the window of no tokens");
    expect(c.is(c.at(1, 3, 0, 3), s3), "multi-byte class ids: the whole sentence");
    expect(c.is(c.at(1, 3, 1, 2), s3.substr(2)), "multi-byte class ids: behind a two-byte token");
    expect(c.is(c.at(1, 3, 2, 1), s3.substr(3)), "multi-byte class ids: a four-byte token at the sentence's end");
    expect(!c.at(1, 3, 1, 3).fits && !c.at(1, 3, 3, 1).fits, "multi-byte class ids: one token too long");
    expect(c.is(c.at(1, 4, 0, 1), "\x0a"), "the last sentence, ended by the payload");
    expect(!c.at(1, 4, 0, 2).fits && !c.at(1, 4, 1, 1).fits, "... and a window past the payload's end");
    expect(!c.at(1, 5, 0, 1).fits && !c.at(1, 0, 0, 1).fits && !c.at(1, 4294967295u, 0, 1).fits, "a sentence beyond the corpus");
    // the same corpus numbered from 5
    expect(c.is(c.at(5, 5, 1, 3), s1.substr(1)) && c.is(c.at(5, 7, 0, 3), s3) && c.is(c.at(5, 8, 0, 1), "\x0a"), "first_sentence 5: the sentences 5 .. 8");
    expect(!c.at(5, 1, 0, 1).fits && !c.at(5, 4, 0, 1).fits && !c.at(5, 9, 0, 1).fits && !c.at(5, 6, 0, 1).fits, "first_sentence 5: before, behind, and the empty one");
    expect(!c.at(4294967295u, 0, 0, 1).fits && c.is(c.at(4294967295u, 4294967295u, 0, 4), s1), "first_sentence at the top of 32 bits");
    // a payload that ends inside a token, and one that ends with a delimiter; the empty corpus
    const Corpus cut(std::string("\x05\x86", 2));
    expect(cut.is(cut.at(1, 1, 0, 1), "\x05") && !cut.at(1, 1, 0, 2).fits && !cut.at(1, 1, 1, 1).fits, "a token cut by the payload's end is no token");
    const Corpus closed(std::string("\x05\x06\x00", 3));
    expect(closed.start.size() == 1 && closed.is(closed.at(1, 1, 0, 2), std::string("\x05\x06", 2)) && !closed.at(1, 1, 0, 3).fits && !closed.at(1, 2, 0, 1).fits,
           "a closing delimiter opens no sentence");
    const Corpus none("");
    expect(none.start.empty() && !none.at(1, 1, 0, 1).fits && !none.at(1, 1, 0, 0).fits, "the empty corpus");
    // a byte 00 behind a high byte belongs to its token (the payload's own rule)
    const Corpus high(std::string("\x85\x00\x06", 3));
    expect(high.start.size() == 1 && high.is(high.at(1, 1, 0, 2), std::string("\x85\x00\x06", 3)) && high.is(high.at(1, 1, 1, 1), "\x06"), "00 as a token's last byte");
    printf("checked %d mismatches %d\n", checked, mismatches);
    return mismatches ? 1 : 0;
}
