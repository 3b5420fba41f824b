// instance_window.h — where the instance of a pattern lies in a class-encoded corpus: the n tokens that start at a reference (sentence, token), as print() with
// instantiate = true writes them behind every reference of a skipgram row (patternmodel.h; the device form: csrc/print.hpp, print_instlen_kernel). No dependency on
// the model classes: tests/instance_window_check.cpp drives it on plain arrays.
#ifndef COLIBRI_AMD_INSTANCE_WINDOW_H
#define COLIBRI_AMD_INSTANCE_WINDOW_H

#include <cstddef>
#include <cstdint>

namespace colibri_host {

struct InstanceWindow {
    size_t begin = 0, bytes = 0;  // payload[begin .. begin + bytes): the window's tokens, no delimiter among them
    bool   fits  = false;         // false: the sentence is not of this corpus, or it ends before token + n
};

/** payload[0 .. nbytes): the corpus (tokens as base-128 bytes, the last of a token below 128; a token 00 ends a sentence). sentencestart[0 .. nsentences): the
 *  byte offset of every sentence, empty ones included; the first of them is numbered first_sentence. Nothing outside the payload is read. */
inline InstanceWindow instance_window(const unsigned char* payload, size_t nbytes, const uint64_t* sentencestart, size_t nsentences, uint32_t first_sentence, uint32_t sentence,
                                      uint32_t token, uint32_t n) {
    InstanceWindow w;
    if (sentence < first_sentence || (uint64_t)sentence - first_sentence >= nsentences) return w;
    size_t i = (size_t)sentencestart[sentence - first_sentence];
    if (i > nbytes) return w;
    // the token that starts at i ends at the first byte below 128; a one-byte token 00 is the sentence's delimiter
    auto skip = [&](uint32_t count) -> bool {
        for (uint32_t k = 0; k < count; ++k) {
            if (i >= nbytes || payload[i] == 0) return false;
            while (i < nbytes && payload[i] >= 128) ++i;
            if (i >= nbytes) return false;  // (a token cut by the payload's end)
            ++i;
        }
        return true;
    };
    if (!skip(token)) return w;
    w.begin = i;
    if (!skip(n)) return w;
    w.bytes = i - w.begin;
    w.fits  = true;
    return w;
}

}  // namespace colibri_host
#endif
