// colibri-classdecode (MI355X build) — a drop-in for the reference's corpus decoder (src/classdecode.cpp): a class-encoded corpus back to
// text. Same options, output and exit codes; an unknown option, on which the reference aborts, is refused with a message and exit status 2,
// and a data file that cannot be read ends with the reference's message and exit status 1 instead of an uncaught exception. The decoding
// itself is ClassDecoder::decodefile, on the GPU (csrc/decode.hpp); the text reaches stdout in the library's output windows.
#include <getopt.h>
#include <sys/stat.h>

#include <cstdlib>
#include <iostream>
#include <string>

#include "patternmodel.h"

namespace {

void usage() {
    std::cerr << "colibri-classdecode (MI355X-native build of the Colibri Core class decoder)\n"
                 "Syntax: colibri-classdecode -f encoded-corpus -c class-file\n"
                 "Description: Decodes an encoded corpus\n\n"
                 "Options:\n"
                 "\t-s \tstart line number (default: 0)\n"
                 "\t-e \tend line number (default: infinite)\n"
                 "The corpus is decoded on the GPU."
              << std::endl;
}

}  // namespace

int main(int argc, char* argv[]) {
    std::string  classfile, corpusfile;
    unsigned int start = 0, end = 0;
    int          c;
    opterr = 0;
    while ((c = getopt(argc, argv, "c:f:hs:e:")) != -1) {
        switch (c) {
            case 'c': classfile = optarg; break;
            case 'f': corpusfile = optarg; break;
            case 's': start = (unsigned int)atoi(optarg); break;
            case 'e': end = (unsigned int)atoi(optarg); break;
            case 'h': usage(); return 0;
            default: std::cerr << "ERROR: Unknown option: -" << (char)optopt << std::endl; return 2;
        }
    }
    if (classfile.empty() || corpusfile.empty()) {
        usage();
        return 2;
    }
    struct stat st;
    if (stat(classfile.c_str(), &st) != 0) {  // (src/classdecoder.cpp:99-103)
        std::cerr << "File does not exist: " << classfile << std::endl;
        return 3;
    }
    try {
        ClassDecoder classdecoder(classfile);
        classdecoder.decodefile(corpusfile, std::cout, start, end);
        std::cout.flush();
        return std::cout.good() ? 0 : 1;
    } catch (const std::exception& e) {
        std::cerr << "colibri-classdecode: " << e.what() << std::endl;
        return 1;
    }
}
