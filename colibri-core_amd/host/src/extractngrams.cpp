// colibri-extractngrams (MI355X build) — a drop-in for the reference's n-gram extractor (src/extractngrams.cpp): a window of n tokens moves over
// every line of the class-encoded data files, and each n-gram is printed as text, in corpus order. Same options and output, with one stated
// departure: the A2 02 signature of a data file is skipped, where the reference reads it as the first token of the first line.
// Where the reference aborts or has no defined behaviour (§6): -n below 1 and an unknown option are refused with a message and exit status 2; a
// data file that cannot be read, or that is not version 2 data, ends with a message and exit status 1; an empty data file prints nothing. The
// text is written on the GPU (csrc/ngrams.hpp) and reaches stdout in the library's output windows.
#include <getopt.h>

#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "classdecoder.h"
#include "common.h"

namespace {

void usage() {
    std::cerr << "Syntax: colibri-extractngrams -n [size] -c classfile datafile datafile2 ..." << std::endl;
    std::cerr << "Description: Simple tool that just extracts n-grams from corpus data (class encoded), i.e. it moves a simple sliding window over the data, and outputs n-grams in the "
                 "order found, it does not generate any pattern models so is very low in memory"
              << std::endl
              << std::endl;
    std::cerr << "Options:" << std::endl;
    std::cerr << "\t-n int   N-gram size" << std::endl;
    std::cerr << "\t-c str   Class file for decoding" << std::endl;
    std::cerr << "The n-grams are written on the GPU (MI355X-native build)." << std::endl;
}

}  // namespace

int main(int argc, char* argv[]) {
    std::string              classfile;
    std::vector<std::string> datafiles;
    long long                n = 3;
    int                      c;
    opterr = 0;
    while ((c = getopt(argc, argv, "c:hn:")) != -1) {
        switch (c) {
            case 'c': classfile = optarg; break;
            case 'n': n = std::atoll(optarg); break;
            case 'h': usage(); return 0;
            default: std::cerr << "ERROR: Unknown option: -" << (char)optopt << std::endl; return 2;
        }
    }
    for (int i = optind; i < argc; ++i) datafiles.push_back(argv[i]);
    if (classfile.empty()) {
        std::cerr << "ERROR: No class file specified! (-c)" << std::endl;
        usage();
        return 2;
    }
    if (n < 1 || n > 0x7FFFFFFF) {
        std::cerr << "ERROR: the n-gram size (-n) must be between 1 and 2147483647" << std::endl;
        return 2;
    }
    try {
        const ClassDecoder classdecoder(classfile);
        colibri_host::extract_ngrams(classdecoder, datafiles, (int)n, std::cout);
        std::cout.flush();
        return std::cout.good() ? 0 : 1;
    } catch (const std::exception& e) {
        std::cout.flush();
        std::cerr << "colibri-extractngrams: " << e.what() << std::endl;
        return 1;
    }
}
