// query_encode_check <class file> <text file>: every line of the text through ClassEncoder::encodestring and buildpattern (allowunknown = true),
// one output line each: "<tokens> <hex of encodestring's bytes | -> <hex of buildpattern's key | -> <ok | throws>", the last word saying what
// encodestring does with the line when unknown words are not allowed. Test infrastructure of tests/test_query.py.
#include <cstdio>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "classencoder.h"

static std::string hex(const unsigned char* p, size_t n) {
    if (n == 0) return "-";
    static const char* d = "0123456789abcdef";
    std::string        s;
    for (size_t i = 0; i < n; ++i) {
        s += d[p[i] >> 4];
        s += d[p[i] & 15];
    }
    return s;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    ClassEncoder  encoder(argv[1]);
    std::ifstream in(argv[2], std::ios::binary);
    std::string   line;
    while (std::getline(in, line)) {
        std::vector<unsigned char> buf(5 * line.size() + 4096);
        unsigned int               ntok = 0;
        const int                  n    = encoder.encodestring(line, buf.data(), true, false, &ntok);
        const Pattern              p    = encoder.buildpattern(line, true);
        bool                       thrown = false;
        try {
            encoder.encodestring(line, buf.data(), false);
        } catch (const UnknownTokenError&) {
            thrown = true;
        }
        std::cout << ntok << " " << hex(buf.data(), (size_t)n) << " " << hex(p.data, p.bytesize()) << " " << (thrown ? "throws" : "ok") << "\n";
    }
    return 0;
}
