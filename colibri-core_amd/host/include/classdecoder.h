// classdecoder.h — class id -> word map, only what printing a model needs.
// reference: include/classdecoder.h (ClassDecoder), src/classdecoder.cpp:20-43 (bytestoint), :84-130 (load), :259-284 (getdataversion),
// :166-244 (decodefile, decodefile_v1, decodefiletostring: on the device, csrc/decode.hpp), :132-138, :240-257 (decodeseq, add, prune).
// The .colibri.cls format is one "<class id>\t<word>" per line.
#ifndef COLIBRI_AMD_CLASSDECODER_H
#define COLIBRI_AMD_CLASSDECODER_H
#include <cstdint>
#include <fstream>
#include <istream>
#include <ostream>
#include <string>
#include <unordered_map>
#include <vector>

/** decodes one little-endian base-128 class id (high bit set on all bytes but the last); integer shifts, no pow() */
unsigned int bytestoint(const unsigned char* a, unsigned int* length = NULL);
/** 2 for files starting with A2 <version>; 1 for header-less v1 data (first byte is a token length) */
unsigned char getdataversion(std::istream& in);

class ClassDecoder {
  public:
    static const unsigned char delimiterclass = 0, boundaryclass = 1, unknownclass = 2, skipclass = 3, flexclass = 4;
    ClassDecoder();
    explicit ClassDecoder(const std::string& filename);
    void load(const std::string& filename);
    bool hasclass(unsigned int cls) const { return classes.count(cls) != 0; }
    const std::string& operator[](unsigned int cls) const;
    size_t size() const { return classes.size(); }
    unsigned int gethighestclass() const { return highestclass; }
    /** the whole map (what the device-side print uploads as its word table) */
    const std::unordered_map<unsigned int, std::string>& words() const { return classes; }

    /** the words of seq's ids; an id without one gives "" (and, as in the reference, is entered into the map with that word) */
    std::vector<std::string> decodeseq(const std::vector<int>& seq);
    /** a .colibri.dat (v2, or v1 with or without its A2 01 header) as text, decoded on the GPU: lines end < L < start are left out as the
     * reference leaves them out; "Processed <n> lines" on stderr unless quiet. Missing / plain-text files: getdataversion's messages, InternalError */
    void decodefile(const std::string& filename, std::ostream& out, unsigned int start = 0, unsigned int end = 0, bool quiet = false);
    /** the rest of an open stream as v1 data (what decodefile does after getdataversion returned 1) */
    void decodefile_v1(std::ifstream& in, std::ostream& out, unsigned int start = 0, unsigned int end = 0, bool quiet = false);
    std::string decodefiletostring(const std::string& filename, unsigned int start = 0, unsigned int end = 0, bool quiet = true);
    void add(const unsigned int cls, const std::string& word);
    /** drops the ids threshold .. gethighestclass() */
    void prune(unsigned int threshold);

  private:
    void decodepayload(const unsigned char* payload, uint64_t nbytes, int version, std::ostream& out, unsigned int start, unsigned int end, bool quiet) const;
    std::unordered_map<unsigned int, std::string> classes;
    unsigned int highestclass;
};

namespace colibri_host {
/** what colibri-extractngrams -n <n> prints for one version 2 .colibri.dat (reference src/extractngrams.cpp): every window of n tokens inside a line
 * as text and a newline, in corpus order, written on the GPU (csrc/ngrams.hpp). The A2 02 signature is skipped (the reference reads it as a token).
 * Returns the rows. A zero-byte file prints nothing. With messages on stderr and InternalError: n < 1, a file that cannot be opened, plain text or
 * version 1 data, a file of 4 GiB or more, a token the decoder refuses, no device (there is no CPU fallback). */
uint64_t extract_ngrams(const ClassDecoder& classdecoder, const std::string& datafile, int n, std::ostream& out);
/** the same for several data files in order, as the command line takes them: the class map is uploaded once. Returns the rows of all of them. */
uint64_t extract_ngrams(const ClassDecoder& classdecoder, const std::vector<std::string>& datafiles, int n, std::ostream& out);
}  // namespace colibri_host
#endif
