// colibri_host.cpp — non-template parts of the C++ face: key-type helpers, corpus / model file formats, and the glue
// that drives libcolibri_hip.so through its C ABI (include/colibri_hip.h). No counting happens here.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <iterator>
#include <map>
#include <mutex>
#include <sstream>

#include "algorithms.h"
#include "patternmodel.h"
#include "spooky_device.hpp"  // the same SpookyHash routine the kernels use, compiled for the host

// The seed entry points are the newest of the device layer's C ABI. This file is also linked against device layers that do not have them (the CPU stand-in of
// tests/standin/): the references are weak, and device_train refuses a seeded run with a message where they are absent, instead of the link failing.
#pragma weak colibri_set_seed
#pragma weak colibri_seed_fetch

// ---------------------------------------------------------------------------------------------------
// key helpers
// ---------------------------------------------------------------------------------------------------
namespace colibri_host {

uint64_t spooky_hash64(const unsigned char* data, size_t len) {
    if (len >= 192) {
        std::cerr << "ERROR: pattern of " << len << " bytes: SpookyHash's long form is not part of this build" << std::endl;
        throw InternalError();
    }
    unsigned char buf[192 + 16] = {0};  // the device routine may read 15 bytes past the key
    std::memcpy(buf, data, len);
    return colibri::spooky64_short(buf, (uint32_t)len);
}

size_t token_count(const unsigned char* data, size_t bytes) {
    size_t n = 0;
    for (size_t i = 0; i < bytes; ++i) n += data[i] < 128;
    return n;
}

size_t key_bytesize(const unsigned char* data) {
    size_t i        = 0;
    bool   prevhigh = false;
    while (prevhigh || data[i] != 0) {
        prevhigh = data[i] >= 128;
        ++i;
    }
    return i;
}

PatternCategory category_of(const unsigned char* data, size_t bytes) {
    bool prevhigh = false;
    for (size_t i = 0; i < bytes; ++i) {
        if (!prevhigh && data[i] == colibri_classes::flexclass) return FLEXGRAM;
        if (!prevhigh && data[i] == colibri_classes::skipclass) return SKIPGRAM;
        prevhigh = data[i] >= 128;
    }
    return NGRAM;
}

std::string decode_key(const unsigned char* data, size_t bytes, const ClassDecoder& decoder) {
    std::string out;
    size_t      i = 0;
    while (i < bytes) {
        unsigned int len = 0;
        const unsigned int cls = bytestoint(data + i, &len);
        if (!out.empty()) out += ' ';
        if (decoder.hasclass(cls)) {
            out += decoder[cls];
        } else {
            out += "{?}";
        }
        i += len;
    }
    return out;
}

}  // namespace colibri_host

Pattern::Pattern(const PatternPointer& pp) {
    if (pp.data == NULL || pp.bytes == 0) {
        data = NULL;
        return;
    }
    if (pp.mask == 0) {
        assign(pp.data, pp.bytes);
        return;
    }
    // skipgram / flexgram: every gapped token becomes one marker byte; adjacent flex gaps collapse (reference src/pattern.cpp:886-908, :1043-1065)
    const bool                 flex = pp.isflexgram();
    std::vector<unsigned char> buf;
    buf.reserve(pp.bytes);
    int  tok     = 0;
    bool prevgap = false;
    size_t start = 0;
    for (size_t i = 0; i < pp.bytes; ++i) {
        if (pp.data[i] < 128) {
            if (pp.isgap(tok)) {
                if (!(flex && prevgap)) buf.push_back(flex ? colibri_classes::flexclass : colibri_classes::skipclass);
                prevgap = true;
            } else {
                buf.insert(buf.end(), pp.data + start, pp.data + i + 1);
                prevgap = false;
            }
            ++tok;
            start = i + 1;
        }
    }
    assign(buf.data(), buf.size());
}

Pattern::Pattern(std::istream& in, bool ignoreeol, const unsigned char version) {
    (void)ignoreeol;
    data            = NULL;
    const Pattern p = colibri_host::read_model_pattern(in, version);
    assign(p.data, p.data ? p.bytesize() : 0);
}

void Pattern::write(std::ostream& out, const unsigned char*) const {
    const size_t s = bytesize();
    if (s > 0) {
        out.write((const char*)data, (std::streamsize)s + 1);
    } else {
        const char null = 0;
        out.write(&null, 1);
    }
}

std::string Pattern::tostring(const ClassDecoder& decoder) const { return data ? colibri_host::decode_key(data, bytesize(), decoder) : std::string(); }

std::string Pattern::tohex() const {
    static const char* d = "0123456789abcdef";
    std::string        s;
    const size_t       b = bytesize();
    for (size_t i = 0; i < b; ++i) {
        s.push_back(d[data[i] >> 4]);
        s.push_back(d[data[i] & 15]);
    }
    return s;
}

namespace colibri_host {
void token_slices(const unsigned char* data, size_t bytes, std::vector<std::string>& out) {
    size_t begin = 0;
    for (size_t i = 0; i < bytes; ++i)
        if (data[i] < 128) {  // a byte under 128 closes a token
            out.emplace_back((const char*)data + begin, i + 1 - begin);
            begin = i + 1;
        }
}
void print_legend(std::ostream& err, bool indexed) {
    err << std::endl << "Legend:" << std::endl;
    err << " - PATTERN    : The pattern, Gaps in skipgrams are represented as {*}. Variable-width gaps in flexgrams are shown using {**}." << std::endl;
    err << " - COUNT      : The occurrence count - the amount of times the pattern occurs in the data" << std::endl;
    if (indexed) {
        err << " - TOKENS     : The number of tokens in the corpus that this pattern covers" << std::endl;
        err << " - COVERAGE   : The number of tokens covered, as a fraction of the total in the corpus" << std::endl;
    } else {
        err << " - TOKENS     : The maximum number of tokens in the corpus that this pattern covers (a projection: count x size, the model is not indexed)" << std::endl;
        err << " - COVERAGE   : The maximum number of tokens covered, as a fraction of the total in the corpus (projection)" << std::endl;
    }
    err << " - CATEGORY   : The pattern type category (ngram,skipgram,flexgram)" << std::endl;
    err << " - SIZE       : The size of the pattern (in tokens)" << std::endl;
    err << " - FREQUENCY  : The frequency of the pattern within its pattern type category and size-class." << std::endl;
    err << " - REFERENCES : A space-delimited list of sentence:token position where the pattern occurs in the data. Sentences start at 1, tokens at 0" << std::endl;
}
void report_legend(std::ostream& err, bool indexed) {
    err << std::endl << "Legend:" << std::endl;
    err << " - PATTERNS    : The number of distinct patterns within the group" << std::endl;
    if (indexed) {
        err << " - TOKENS      : The number of tokens that is covered by the patterns in the group." << std::endl;
        err << " - COVERAGE    : The number of tokens covered, as a fraction of the total in the corpus" << std::endl;
    }
    err << " - TYPES       : The number of unique *word/unigram* types in this group" << std::endl;
    err << " - OCCURRENCES : The total number of occurrences of the patterns in this group" << std::endl;
}
}  // namespace colibri_host

int PatternPointer::ngrams(std::vector<std::pair<PatternPointer, int>>& container, const int n) const {
    std::vector<size_t> starts{0};
    for (size_t i = 0; i < bytes; ++i)
        if (data[i] < 128) starts.push_back(i + 1);
    const int ntok = (int)starts.size() - 1;
    if (n > ntok) return 0;
    for (int i = 0; i + n <= ntok; ++i) container.push_back(std::make_pair(PatternPointer(data + starts[i], starts[i + n] - starts[i]), i));
    return ntok - n + 1;
}
int PatternPointer::ngrams(std::vector<PatternPointer>& container, const int n) const {
    std::vector<std::pair<PatternPointer, int>> tmp;
    const int                                   r = ngrams(tmp, n);
    for (const auto& p : tmp) container.push_back(p.first);
    return r;
}
namespace {
// the sizes minn..maxn one after the other, each through the container's own ngrams()
template <class Source, class Container>
int sub_windows(const Source& src, Container& container, int minn, int maxn) {
    const int ntok = (int)src.n();
    if (maxn > ntok) maxn = ntok;
    if (minn > ntok) return 0;
    int found = 0;
    for (int k = minn; k <= maxn; ++k) found += src.ngrams(container, k);
    return found;
}
}  // namespace
int PatternPointer::subngrams(std::vector<PatternPointer>& container, int minn, int maxn) const { return sub_windows(*this, container, minn, maxn); }
int PatternPointer::subngrams(std::vector<std::pair<PatternPointer, int>>& container, int minn, int maxn) const { return sub_windows(*this, container, minn, maxn); }

// Pattern: the windows are views into (or copies of) this pattern's own bytes; a gap token (the byte 03) stays what it is
int Pattern::ngrams(std::vector<std::pair<PatternPointer, int>>& container, const int n) const {
    if (data == NULL) return 0;
    return PatternPointer(data, bytesize()).ngrams(container, n);
}
int Pattern::ngrams(std::vector<PatternPointer>& container, const int n) const {
    if (data == NULL) return 0;
    return PatternPointer(data, bytesize()).ngrams(container, n);
}
int Pattern::ngrams(std::vector<std::pair<Pattern, int>>& container, const int n) const {
    std::vector<std::pair<PatternPointer, int>> tmp;
    const int                                   r = ngrams(tmp, n);
    for (const auto& p : tmp) container.push_back(std::make_pair(Pattern(p.first.data, p.first.bytes), p.second));
    return r;
}
int Pattern::ngrams(std::vector<Pattern>& container, const int n) const {
    std::vector<std::pair<PatternPointer, int>> tmp;
    const int                                   r = ngrams(tmp, n);
    for (const auto& p : tmp) container.push_back(Pattern(p.first.data, p.first.bytes));
    return r;
}
int Pattern::subngrams(std::vector<Pattern>& container, int minn, int maxn) const { return sub_windows(*this, container, minn, maxn); }
int Pattern::subngrams(std::vector<PatternPointer>& container, int minn, int maxn) const { return sub_windows(*this, container, minn, maxn); }
int Pattern::subngrams(std::vector<std::pair<Pattern, int>>& container, int minn, int maxn) const { return sub_windows(*this, container, minn, maxn); }
int Pattern::subngrams(std::vector<std::pair<PatternPointer, int>>& container, int minn, int maxn) const { return sub_windows(*this, container, minn, maxn); }

// ---------------------------------------------------------------------------------------------------
// gap masks (algorithms.h)
// ---------------------------------------------------------------------------------------------------
uint32_t vector2mask(const std::vector<std::pair<int, int>>& skips) {
    uint32_t mask = 0;
    for (const auto& gap : skips)
        for (int i = gap.first; i < gap.first + gap.second && i < 31; ++i) mask |= bitmask_of(i);
    return mask;
}
std::vector<std::pair<int, int>> mask2vector(const uint32_t mask, const int n) {
    std::vector<std::pair<int, int>> gaps;
    int                              k = 0;
    while (k < n) {
        if (!(mask & bitmask_of(k))) {
            ++k;
            continue;
        }
        const int begin = k;
        while (k < n && (mask & bitmask_of(k))) ++k;
        gaps.push_back(std::make_pair(begin, k - begin));
    }
    return gaps;
}
std::vector<std::pair<int, int>> get_consecutive_gaps(const int n, const int leftmargin, const int rightmargin) {
    std::vector<std::pair<int, int>> gaps;
    for (int begin = leftmargin; begin < n; ++begin)
        for (int length = (n - rightmargin) - begin; length > 0; --length) gaps.push_back(std::make_pair(begin, length));
    return gaps;
}
uint32_t reversemask(uint32_t mask, const unsigned int n) {
    const uint32_t inverted = ~mask;
    return n >= 32 ? 0u : (uint32_t)(inverted << n) >> n;  // the reference's arithmetic: n bits up, n bits down, in 32 bits
}
int maskheadskip(uint32_t mask, const unsigned int) {
    unsigned int i = 0;
    while (i < 31 && (mask & bitmask_of((int)i))) ++i;
    return (int)i;
}
int masktailskip(uint32_t mask, const unsigned int n) {
    unsigned int i = 0;
    while (i < n && (mask & bitmask_of((int)(n - i - 1)))) ++i;
    return (int)i;
}
std::vector<uint32_t> compute_skip_configurations(const int n, const int maxskips) {
    std::vector<uint32_t> masks;
    if (n < 3 || n > 32) return masks;  // (a gap mask is a uint32_t that covers neither end: beyond 32 tokens the reference's own loop is undefined)
    for (uint32_t inner = 1; inner < (uint32_t(1) << (n - 2)); ++inner) {
        const uint32_t mask = inner << 1;  // never the first or the last token
        if (n - 2 >= maxskips && mask2vector(mask, n).size() > (size_t)maxskips) continue;
        masks.push_back(mask);
    }
    return masks;
}

// ---------------------------------------------------------------------------------------------------
// class decoding
// ---------------------------------------------------------------------------------------------------
unsigned int bytestoint(const unsigned char* a, unsigned int* length) {
    unsigned int result = 0, i = 0;
    for (;; ++i) {
        const unsigned char b = a[i];
        if (i < 5) result |= (unsigned int)(b & 127) << (7 * i);
        if (b < 128) break;
    }
    if (length) *length = i + 1;
    return result;
}

unsigned char getdataversion(std::istream& in) {
    if (!in.good()) {
        std::cerr << "ERROR: Supplied data file can not be opened. Check whether it exists and whether you have proper permissions..." << std::endl;
        throw InternalError();
    }
    in.clear();
    in.seekg(0);
    unsigned char b = 0, version = 1;
    in.read((char*)&b, 1);
    if (b == 0xa2) {
        in.read((char*)&version, 1);
    } else {
        if (b > 5 && in.gcount() == 1) {
            std::cerr << "ERROR: Supplied data file is not a valid Colibri Data file, did you pass plain-text instead perhaps?..." << std::endl;
            throw InternalError();
        }
        in.clear();
        in.seekg(0);
    }
    return version;
}

ClassDecoder::ClassDecoder() : highestclass(0) {
    classes[unknownclass] = "{?}";
    classes[skipclass]    = "{*}";
    classes[flexclass]    = "{**}";
    classes[boundaryclass] = "{|}";
}
ClassDecoder::ClassDecoder(const std::string& filename) : ClassDecoder() { load(filename); }
void ClassDecoder::load(const std::string& filename) {
    std::ifstream in(filename);
    if (!in.good()) {
        std::cerr << "ERROR: Unable to load class file " << filename << std::endl;
        throw InternalError();
    }
    std::string line;
    while (std::getline(in, line)) {
        const size_t tab = line.find('\t');
        if (tab == std::string::npos) continue;
        const unsigned int cls = (unsigned int)std::strtoul(line.substr(0, tab).c_str(), NULL, 10);
        classes[cls]           = line.substr(tab + 1);
        if (cls > highestclass) highestclass = cls;
    }
}
const std::string& ClassDecoder::operator[](unsigned int cls) const {
    static const std::string unknown = "{?}";
    auto                     it      = classes.find(cls);
    return it == classes.end() ? unknown : it->second;
}

// ---------------------------------------------------------------------------------------------------
// corpus files
// ---------------------------------------------------------------------------------------------------
namespace colibri_host {

// v1: token = length byte (1..127) + little-endian base-256 digits; 00 ends a sentence; 128/129 = skip/flex markers
static std::vector<unsigned char> v1_to_v2(const std::vector<unsigned char>& in) {
    std::vector<unsigned char> out;
    out.reserve(in.size());
    size_t i = 0;
    while (i < in.size()) {
        const unsigned char c = in[i];
        if (c == 0) {
            out.push_back(0);
            ++i;
        } else if (c < 128) {
            if (i + 1 + c > in.size()) {
                std::cerr << "ERROR: Invalid pattern data, unexpected end of file" << std::endl;
                throw InternalError();
            }
            uint32_t cls = 0;
            for (unsigned k = 0; k < c && k < 4; ++k) cls |= (uint32_t)in[i + 1 + k] << (8 * k);
            do {
                unsigned char b = cls & 127;
                cls >>= 7;
                if (cls) b |= 128;
                out.push_back(b);
            } while (cls);
            i += (size_t)c + 1;
        } else {
            if (c == 128) out.push_back(colibri_classes::skipclass);
            if (c == 129) out.push_back(colibri_classes::flexclass);
            ++i;
        }
    }
    return out;
}

std::vector<unsigned char> read_corpus_payload(std::istream& in) {
    const unsigned char version = getdataversion(in);  // leaves the stream after the 2-byte header for v2, at 0 for v1
    std::vector<unsigned char> raw((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    if (version >= 2) return raw;
    return v1_to_v2(raw);
}

Pattern read_model_pattern(std::istream& in, unsigned char classencodingversion) {
    std::vector<unsigned char> buf;
    unsigned char              c = 0;
    if (classencodingversion == 1) {
        while (in.read((char*)&c, 1)) {
            buf.push_back(c);
            if (c == 0) break;
            if (c < 128) {
                for (unsigned k = 0; k < c; ++k) {
                    unsigned char d = 0;
                    in.read((char*)&d, 1);
                    buf.push_back(d);
                }
            }
        }
        std::vector<unsigned char> v2 = v1_to_v2(buf);
        if (!v2.empty() && v2.back() == 0) v2.pop_back();
        return Pattern(v2.data(), v2.size());
    }
    bool prevhigh = false;
    while (in.read((char*)&c, 1)) {
        if (!prevhigh && c == 0) break;
        buf.push_back(c);
        prevhigh = c >= 128;
    }
    return Pattern(buf.data(), buf.size());
}

// ---------------------------------------------------------------------------------------------------
// driving the device library
// ---------------------------------------------------------------------------------------------------
namespace {
struct CtxGuard {
    colibri_ctx* c = nullptr;
    ~CtxGuard() { colibri_destroy(c); }
};
// One idle device context per GPU is kept between plain train() calls of a process: creating a context, reserving its working buffers in HBM and releasing them again
// cost ~15 ms of a ~34 ms call on a 10^8-token corpus (COLIBRI_HOST_TIMING=1), and a caller that trains model after model pays them every time. A context that ran
// with a constraint / filter / continuation set, or that failed, is never returned here. The cached context is not destroyed at exit (the HIP runtime may already be
// gone when static destructors run; the driver reclaims the memory). COLIBRI_CTX_CACHE=0 turns this off.
struct CtxCache {
    std::mutex                  m;
    std::map<int, colibri_ctx*> idle;
    static CtxCache& get() {
        static CtxCache* c = new CtxCache;  // (leaked on purpose, see above)
        return *c;
    }
    static bool on() {
        static const bool v = [] {
            const char* e = std::getenv("COLIBRI_CTX_CACHE");
            return !(e && e[0] == '0');
        }();
        return v;
    }
    colibri_ctx* take(int device) {
        if (!on()) return nullptr;
        std::lock_guard<std::mutex> l(m);
        auto                        it = idle.find(device);
        if (it == idle.end()) return nullptr;
        colibri_ctx* c = it->second;
        idle.erase(it);
        return c;
    }
    void evict(int device) {  // device < 0: every device's
        std::vector<colibri_ctx*> gone;
        {
            std::lock_guard<std::mutex> l(m);
            for (auto it = idle.begin(); it != idle.end();) {
                if (device < 0 || it->first == device) {
                    gone.push_back(it->second);
                    it = idle.erase(it);
                } else {
                    ++it;
                }
            }
        }
        for (colibri_ctx* c : gone) colibri_destroy(c);
    }
    void give(int device, colibri_ctx* c) {  // takes ownership
        if (c == nullptr) return;
        if (on()) {
            std::lock_guard<std::mutex> l(m);
            if (idle.find(device) == idle.end()) {
                idle[device] = c;
                return;
            }
        }
        colibri_destroy(c);
    }
};
// The arrays of the last released result (one set per process) wait for the next export: 150 MB of keys / offsets / counts for a 10^8-token model are ~37 000 fresh
// pages otherwise — 27-31 ms of page faults per train() once nothing else keeps the heap warm, twice the device work. They are handed over with their old size (no
// zero fill: the export overwrites every element). COLIBRI_RESULT_POOL=0 turns this off.
struct ResultPool {
    std::mutex                 m;
    bool                       full = false;
    std::vector<uint64_t>      key_off, ref_off;
    std::vector<unsigned char> key_bytes;
    std::vector<uint32_t>      counts, ref_sentence;
    std::vector<uint16_t>      ref_token;
    static ResultPool& get() {
        static ResultPool* p = new ResultPool;  // (leaked on purpose: released models may outlive static destructors)
        return *p;
    }
    static bool on() {
        static const bool v = [] {
            const char* e = std::getenv("COLIBRI_RESULT_POOL");
            return !(e && e[0] == '0');
        }();
        return v;
    }
};
void take_result_buffers(TrainResult& out) {
    if (!ResultPool::on()) return;
    ResultPool&                 p = ResultPool::get();
    std::lock_guard<std::mutex> l(p.m);
    if (!p.full) return;
    out.key_off.swap(p.key_off);
    out.key_bytes.swap(p.key_bytes);
    out.counts.swap(p.counts);
    out.ref_off.swap(p.ref_off);
    out.ref_sentence.swap(p.ref_sentence);
    out.ref_token.swap(p.ref_token);
    p.full = false;
}
[[noreturn]] void raise(colibri_ctx* c, int rc, const char* what) {
    std::cerr << "ERROR: " << what << " failed (status " << rc << "): " << (c ? colibri_last_error(c) : "no MI355X / HIP device available; there is no CPU fallback") << std::endl;
    throw InternalError();
}
// A fresh context on COLIBRI_DEVICE for one call on a loaded model. false (only when !loud): no usable device, and the caller's host path stands in.
bool open_context(CtxGuard& g, bool loud = true) {
    const char* dev = std::getenv("COLIBRI_DEVICE");
    const int   rc  = colibri_create(&g.c, dev ? std::atoi(dev) : 0);
    if (rc == COLIBRI_OK) return true;
    if (!loud) return false;
    raise(nullptr, rc, "colibri_create");
}
// the same with the corpus that the call reads
bool open_context(CtxGuard& g, const unsigned char* payload, uint64_t nbytes, bool loud = true) {
    if (!open_context(g, loud)) return false;
    const int rc = colibri_upload_corpus(g.c, payload, nbytes, 1);
    if (rc != COLIBRI_OK) raise(g.c, rc, "colibri_upload_corpus");
    return true;
}
// the context a model was kept on while its resident model is still the host's; null once the host arrays were edited after the run
colibri_ctx* resident_context(const std::shared_ptr<void>& device, const TrainResult& model) {
    colibri_ctx* c  = static_cast<colibri_ctx*>(device.get());
    uint64_t     np = 0;
    return model.device_current && colibri_result_sizes(c, &np, NULL, NULL) == COLIBRI_OK && np == model.size() ? c : nullptr;
}
// the device library takes a pointer even for an array of no elements: one zero element stands in
template <class T>
const T* or_none(const T* p) {
    static const T none = 0;
    return p ? p : &none;
}
}  // namespace

namespace {
void fetch_flexgrams(colibri_ctx* c, uint64_t nf, uint64_t kb, uint64_t nr, TrainResult& out) {
    out.key_off.assign(nf + 1, 0);
    out.key_bytes.assign(kb + 1, 0);
    out.counts.assign(nf + 1, 0);
    out.ref_off.assign(nf + 1, 0);
    out.ref_sentence.assign(nr + 1, 0);
    out.ref_token.assign(nr + 1, 0);
    const int rc = colibri_flexgrams_fetch(c, out.key_off.data(), out.key_bytes.data(), out.counts.data(), out.ref_off.data(), out.ref_sentence.data(), out.ref_token.data());
    if (rc != COLIBRI_OK) raise(c, rc, "colibri_flexgrams_fetch");
    out.counts.resize(nf);
}
}  // namespace

void device_flexgrams_resident(const std::shared_ptr<void>& device, TrainResult& out) {
    colibri_ctx* c  = static_cast<colibri_ctx*>(device.get());
    uint64_t     nf = 0, kb = 0, nr = 0;
    const int    rc = colibri_flexgrams_resident(c, &nf, &kb, &nr);
    if (rc != COLIBRI_OK) raise(c, rc, "colibri_flexgrams_resident");
    fetch_flexgrams(c, nf, kb, nr, out);
}

// The co-occurrence entry points are referenced weakly: the CPU stand-in of the device layer that the multi-GPU driver's tests link instead of
// libcolibri_hip.so (tests/standin) does not implement them, and a call there fails with a message instead of the link.
extern "C" {
int colibri_cooc(colibri_ctx*, const uint64_t*, const uint8_t*, const uint64_t*, const uint32_t*, const uint16_t*, uint64_t, uint32_t, int, double, uint64_t*) __attribute__((weak));
int colibri_cooc_resident(colibri_ctx*, uint32_t, int, double, uint64_t*) __attribute__((weak));
int colibri_cooc_fetch(colibri_ctx*, uint32_t*, uint32_t*, uint32_t*, double*) __attribute__((weak));
}
namespace {
void need_cooc() {
    if (colibri_cooc && colibri_cooc_resident && colibri_cooc_fetch) return;
    std::cerr << "ERROR: this build's device layer has no co-occurrence entry points" << std::endl;
    throw InternalError();
}
void fetch_cooc(colibri_ctx* c, uint64_t n, CoocRows& out) {
    out.a.assign(n + 1, 0);
    out.b.assign(n + 1, 0);
    out.count.assign(n + 1, 0);
    out.value.assign(n + 1, 0.0);
    const int rc = colibri_cooc_fetch(c, out.a.data(), out.b.data(), out.count.data(), out.value.data());
    if (rc != COLIBRI_OK) raise(c, rc, "colibri_cooc_fetch");
    out.a.resize(n);
    out.b.resize(n);
    out.count.resize(n);
    out.value.resize(n);
}
}  // namespace

void device_cooc(const std::vector<uint64_t>& key_off, const unsigned char* key_bytes, const std::vector<uint64_t>& ref_off, const uint32_t* ref_sentence, const uint16_t* ref_token,
                 const unsigned char* payload, uint64_t nbytes, uint32_t threshold, int mode, double npmi_threshold, CoocRows& out) {
    need_cooc();
    CtxGuard g;
    open_context(g, payload, nbytes);
    const uint64_t np = key_off.empty() ? 0 : key_off.size() - 1;
    uint64_t       n  = 0;
    const int rc = colibri_cooc(g.c, key_off.data(), or_none(key_bytes), ref_off.data(), or_none(ref_sentence), or_none(ref_token), np, threshold, mode, npmi_threshold, &n);
    if (rc != COLIBRI_OK) raise(g.c, rc, "colibri_cooc");
    fetch_cooc(g.c, n, out);
}

bool device_cooc_resident(const std::shared_ptr<void>& device, const TrainResult& model, uint32_t threshold, int mode, double npmi_threshold, CoocRows& out) {
    need_cooc();
    colibri_ctx* c = resident_context(device, model);
    if (!c) return false;
    uint64_t  n  = 0;
    const int rc = colibri_cooc_resident(c, threshold, mode, npmi_threshold, &n);
    if (rc != COLIBRI_OK) raise(c, rc, "colibri_cooc_resident");
    fetch_cooc(c, n, out);
    return true;
}

// The relation entry points are referenced weakly, as the co-occurrence ones are (tests/standin does not implement them).
extern "C" {
int colibri_relations(colibri_ctx*, const uint64_t*, const uint8_t*, const uint64_t*, const uint32_t*, const uint16_t*, uint64_t, int, uint32_t, uint64_t*) __attribute__((weak));
int colibri_relations_resident(colibri_ctx*, int, uint32_t, uint64_t*) __attribute__((weak));
int colibri_relations_fetch(colibri_ctx*, uint32_t*, uint32_t*, uint32_t*) __attribute__((weak));
}
namespace {
void need_relations() {
    if (colibri_relations && colibri_relations_resident && colibri_relations_fetch) return;
    std::cerr << "ERROR: this build's device layer has no relation entry points" << std::endl;
    throw InternalError();
}
void fetch_relations(colibri_ctx* c, uint64_t n, RelationRows& out) {
    out.a.assign(n + 1, 0);
    out.b.assign(n + 1, 0);
    out.count.assign(n + 1, 0);
    const int rc = colibri_relations_fetch(c, out.a.data(), out.b.data(), out.count.data());
    if (rc != COLIBRI_OK) raise(c, rc, "colibri_relations_fetch");
    out.a.resize(n);
    out.b.resize(n);
    out.count.resize(n);
}
}  // namespace

void device_relations(const std::vector<uint64_t>& key_off, const unsigned char* key_bytes, const std::vector<uint64_t>& ref_off, const uint32_t* ref_sentence,
                      const uint16_t* ref_token, const unsigned char* payload, uint64_t nbytes, int kind, uint32_t threshold, RelationRows& out) {
    need_relations();
    CtxGuard g;
    open_context(g, payload, nbytes);
    const uint64_t np = key_off.empty() ? 0 : key_off.size() - 1;
    uint64_t       n  = 0;
    const int rc = colibri_relations(g.c, key_off.data(), or_none(key_bytes), ref_off.data(), or_none(ref_sentence), or_none(ref_token), np, kind, threshold, &n);
    if (rc != COLIBRI_OK) raise(g.c, rc, "colibri_relations");
    fetch_relations(g.c, n, out);
}

bool device_relations_resident(const std::shared_ptr<void>& device, const TrainResult& model, int kind, uint32_t threshold, RelationRows& out) {
    need_relations();
    colibri_ctx* c = resident_context(device, model);
    if (!c) return false;
    uint64_t  n  = 0;
    const int rc = colibri_relations_resident(c, kind, threshold, &n);
    if (rc != COLIBRI_OK) raise(c, rc, "colibri_relations_resident");
    fetch_relations(c, n, out);
    return true;
}

// The skip-content entry points are referenced weakly too.
extern "C" {
int colibri_skipcontent(colibri_ctx*, const uint64_t*, const uint8_t*, const uint64_t*, const uint32_t*, const uint16_t*, uint64_t, uint64_t*, uint64_t*) __attribute__((weak));
int colibri_skipcontent_resident(colibri_ctx*, uint64_t*, uint64_t*) __attribute__((weak));
int colibri_skipcontent_fetch(colibri_ctx*, uint32_t*, uint32_t*, uint32_t*, uint64_t*, uint8_t*) __attribute__((weak));
}
namespace {
void need_skipcontent() {
    if (colibri_skipcontent && colibri_skipcontent_resident && colibri_skipcontent_fetch) return;
    std::cerr << "ERROR: this build's device layer has no skip-content entry points" << std::endl;
    throw InternalError();
}
void fetch_skipcontent(colibri_ctx* c, uint64_t n, uint64_t nbytes, SkipContentRows& out) {
    out.a.assign(n + 1, 0);
    out.b.assign(n + 1, 0);
    out.count.assign(n + 1, 0);
    out.content_off.assign(n + 1, 0);
    out.content_bytes.assign(nbytes + 1, 0);
    const int rc = colibri_skipcontent_fetch(c, out.a.data(), out.b.data(), out.count.data(), out.content_off.data(), out.content_bytes.data());
    if (rc != COLIBRI_OK) raise(c, rc, "colibri_skipcontent_fetch");
    out.a.resize(n);
    out.b.resize(n);
    out.count.resize(n);
}
}  // namespace

void device_skipcontent(const std::vector<uint64_t>& key_off, const unsigned char* key_bytes, const std::vector<uint64_t>& ref_off, const uint32_t* ref_sentence,
                        const uint16_t* ref_token, const unsigned char* payload, uint64_t nbytes, SkipContentRows& out) {
    need_skipcontent();
    CtxGuard g;
    open_context(g, payload, nbytes);
    const uint64_t np = key_off.empty() ? 0 : key_off.size() - 1;
    uint64_t       n = 0, nb = 0;
    const int rc = colibri_skipcontent(g.c, key_off.data(), or_none(key_bytes), ref_off.data(), or_none(ref_sentence), or_none(ref_token), np, &n, &nb);
    if (rc != COLIBRI_OK) raise(g.c, rc, "colibri_skipcontent");
    fetch_skipcontent(g.c, n, nb, out);
}

bool device_skipcontent_resident(const std::shared_ptr<void>& device, const TrainResult& model, SkipContentRows& out) {
    need_skipcontent();
    colibri_ctx* c = resident_context(device, model);
    if (!c) return false;
    uint64_t  n = 0, nb = 0;
    const int rc = colibri_skipcontent_resident(c, &n, &nb);
    if (rc != COLIBRI_OK) raise(c, rc, "colibri_skipcontent_resident");
    fetch_skipcontent(c, n, nb, out);
    return true;
}

// The comparison entry points are referenced weakly, as the relation ones are.
extern "C" {
int colibri_compare(colibri_ctx*, int, const uint64_t* const*, const uint8_t* const*, const uint32_t* const*, const uint64_t*, const uint64_t*, int, uint64_t*) __attribute__((weak));
int colibri_compare_fetch(colibri_ctx*, uint32_t*, uint32_t*, double*, uint32_t*, uint32_t*) __attribute__((weak));
}

void device_compare(const std::vector<CompareInput>& models, bool conjunctiononly, bool sorted, CompareRows& out) {
    if (!colibri_compare || !colibri_compare_fetch) {
        std::cerr << "ERROR: this build's device layer has no comparison entry points" << std::endl;
        throw InternalError();
    }
    const size_t N = models.size();
    for (size_t m = 0; m < N; ++m)
        if (models[m].tokens > 0x7FFFFFFFull) {  // (refused before any device work: the reference's int totals would wrap)
            std::cerr << "ERROR: model " << m << " has " << models[m].tokens << " tokens; comparing models of more than 2147483647 tokens is not supported" << std::endl;
            throw InternalError();
        }
    std::vector<const uint64_t*> off(N);
    std::vector<const uint8_t*>  bytes(N);
    std::vector<const uint32_t*> counts(N);
    std::vector<uint64_t>        np(N), tok(N);
    static const uint64_t        zero_off = 0;
    static const uint8_t         none     = 0;
    static const uint32_t        c0       = 0;
    for (size_t m = 0; m < N; ++m) {
        np[m]     = models[m].npatterns;
        tok[m]    = models[m].tokens;
        off[m]    = models[m].key_off ? models[m].key_off : &zero_off;
        bytes[m]  = models[m].key_bytes ? models[m].key_bytes : &none;
        counts[m] = models[m].counts ? models[m].counts : &c0;
    }
    CtxGuard    g;
    const char* dev = std::getenv("COLIBRI_DEVICE");
    int         rc  = colibri_create(&g.c, dev ? std::atoi(dev) : 0);
    if (rc != COLIBRI_OK) raise(nullptr, rc, "colibri_create");
    uint64_t n = 0;
    const int flags = (conjunctiononly ? COLIBRI_COMPARE_CONJUNCTION : 0) | (sorted ? 0 : COLIBRI_COMPARE_UNSORTED);
    if ((rc = colibri_compare(g.c, (int)N, off.data(), bytes.data(), counts.data(), np.data(), tok.data(), flags, &n)) != COLIBRI_OK) raise(g.c, rc, "colibri_compare");
    out.nmodels = N;
    out.model.assign(n + 1, 0);
    out.index.assign(n + 1, 0);
    out.ll.assign(n + 1, 0.0);
    out.observed.assign(n * N + 1, 0);
    out.group_totals.assign(n * N + 1, 0);
    if ((rc = colibri_compare_fetch(g.c, out.model.data(), out.index.data(), out.ll.data(), out.observed.data(), out.group_totals.data())) != COLIBRI_OK)
        raise(g.c, rc, "colibri_compare_fetch");
    out.model.resize(n);
    out.index.resize(n);
    out.ll.resize(n);
    out.observed.resize(n * N);
    out.group_totals.resize(n * N);
}

// The coverage entry points are referenced weakly, as the comparison ones are.
extern "C" {
int colibri_coverage(colibri_ctx*, const uint64_t*, const uint8_t*, const uint32_t*, const uint64_t*, const uint32_t*, const uint16_t*, uint64_t, int, uint64_t*) __attribute__((weak));
int colibri_coverage_resident(colibri_ctx*, int, uint64_t*) __attribute__((weak));
int colibri_coverage_fetch(colibri_ctx*, uint64_t*, uint64_t*, uint64_t*, uint64_t*) __attribute__((weak));
}

ReportMode report_mode() {
    const char* e = std::getenv("COLIBRI_REPORT");
    if (e && std::strcmp(e, "host") == 0) return REPORT_HOST;
    if (e && std::strcmp(e, "device") == 0) return REPORT_DEVICE;
    return REPORT_AUTO;
}
uint64_t report_min_work() {
    const char*     e = std::getenv("COLIBRI_REPORT_MIN");
    const long long v = e ? std::atoll(e) : 0;
    return v > 0 ? (uint64_t)v : 2000000ull;
}

namespace {
// after a coverage call: the values, or (only under REPORT_AUTO, only for a refusal the host path stands in for) false
bool fetch_coverage(colibri_ctx* c, int rc, const char* what, uint64_t G, bool loud, CoverageGroups& out) {
    if (rc == COLIBRI_ERR_OVERFLOW && !loud) return false;
    if (rc != COLIBRI_OK) raise(c, rc, what);
    out.G = (uint32_t)G;
    out.patterns.assign(4 * G + 1, 0);
    out.counts.assign(4 * G + 1, 0);
    out.types.assign(4 * G + 1, 0);
    out.tokens.assign(4 * G + 1, 0);
    if ((rc = colibri_coverage_fetch(c, out.patterns.data(), out.counts.data(), out.types.data(), out.tokens.data())) != COLIBRI_OK) raise(c, rc, "colibri_coverage_fetch");
    return true;
}
bool have_coverage(bool loud) {
    if (colibri_coverage && colibri_coverage_resident && colibri_coverage_fetch) return true;
    if (!loud) return false;
    std::cerr << "ERROR: this build's device layer has no coverage entry points" << std::endl;
    throw InternalError();
}
}  // namespace

bool device_coverage(const uint64_t* key_off, const unsigned char* key_bytes, const uint32_t* counts, const uint64_t* ref_off, const uint32_t* ref_sentence, const uint16_t* ref_token,
                     uint64_t npatterns, bool tokens, bool loud, CoverageGroups& out) {
    if (!have_coverage(loud)) return false;
    CtxGuard g;
    if (!open_context(g, loud)) return false;
    uint64_t  G  = 0;
    const int rc = colibri_coverage(g.c, key_off, or_none(key_bytes), counts, ref_off, ref_sentence, ref_token, npatterns, tokens ? 0 : COLIBRI_COV_NO_TOKENS, &G);
    if (rc == COLIBRI_ERR_OVERFLOW && !loud) std::cerr << "(coverage on the host: " << colibri_last_error(g.c) << ")" << std::endl;
    return fetch_coverage(g.c, rc, "colibri_coverage", G, loud, out);
}

bool device_coverage_resident(const std::shared_ptr<void>& device, const TrainResult& model, bool tokens, bool loud, CoverageGroups& out) {
    if (!have_coverage(loud)) return false;
    colibri_ctx* c = resident_context(device, model);
    uint64_t     G = 0;
    if (!c) return false;
    const int rc = colibri_coverage_resident(c, tokens ? 0 : COLIBRI_COV_NO_TOKENS, &G);
    if (rc == COLIBRI_ERR_STATE) return false;  // (not an indexed single-device run: the uploaded form)
    if (rc == COLIBRI_ERR_OVERFLOW && !loud) std::cerr << "(coverage on the host: " << colibri_last_error(c) << ")" << std::endl;
    return fetch_coverage(c, rc, "colibri_coverage_resident", G, loud, out);
}

// The print / histogram entry points are referenced weakly, as the coverage ones are.
extern "C" {
int colibri_print_classes(colibri_ctx*, const uint64_t*, const uint8_t*, const uint8_t*, uint64_t) __attribute__((weak));
int colibri_print_model(colibri_ctx*, const uint64_t*, const uint8_t*, const uint32_t*, const uint64_t*, const uint32_t*, const uint16_t*, uint64_t, uint64_t, colibri_decode_sink, void*,
                        uint64_t*) __attribute__((weak));
int colibri_print_model_resident(colibri_ctx*, uint64_t, colibri_decode_sink, void*, uint64_t*) __attribute__((weak));
int colibri_print_instances(colibri_ctx*, const uint64_t*, const uint8_t*, const uint32_t*, const uint64_t*, const uint32_t*, const uint16_t*, uint64_t, uint64_t, colibri_decode_sink,
                            void*, uint64_t*) __attribute__((weak));
int colibri_print_instances_resident(colibri_ctx*, uint64_t, colibri_decode_sink, void*, uint64_t*) __attribute__((weak));
int colibri_histogram(colibri_ctx*, const uint64_t*, const uint8_t*, const uint32_t*, const uint64_t*, uint64_t, int, uint64_t, uint64_t*) __attribute__((weak));
int colibri_histogram_resident(colibri_ctx*, int, uint64_t, uint64_t*) __attribute__((weak));
int colibri_histogram_fetch(colibri_ctx*, uint32_t*, uint64_t*) __attribute__((weak));
}

namespace {
ReportMode mode_from(const char* var) {
    const char* e = std::getenv(var);
    if (e && std::strcmp(e, "host") == 0) return REPORT_HOST;
    if (e && std::strcmp(e, "device") == 0) return REPORT_DEVICE;
    return REPORT_AUTO;
}
}  // namespace
ReportMode print_mode() { return mode_from("COLIBRI_PRINT"); }
ReportMode histogram_mode() { return mode_from("COLIBRI_HISTOGRAM"); }
uint64_t   print_min_work() {
    const char*     e = std::getenv("COLIBRI_PRINT_MIN");
    const long long v = e ? std::atoll(e) : 0;
    return v > 0 ? (uint64_t)v : ~0ull;  // (no measured break-even yet, DESIGN.md §5f: without the variable, auto stays on the host path)
}
bool stream_in_default_float_state(const std::ostream& out) {
    const std::ios::fmtflags f = out.flags();
    return out.precision() == 6 && out.width() == 0 && !(f & (std::ios::fixed | std::ios::scientific | std::ios::showpoint | std::ios::uppercase | std::ios::showpos));
}

namespace {
bool have_print(bool loud) {
    if (colibri_print_classes && colibri_print_model && colibri_print_model_resident && colibri_histogram && colibri_histogram_resident && colibri_histogram_fetch) return true;
    if (!loud) return false;
    std::cerr << "ERROR: this build's device layer has no print / histogram entry points" << std::endl;
    throw InternalError();
}
bool have_instances(bool loud) {
    if (colibri_print_instances && colibri_print_instances_resident) return true;
    if (!loud) return false;
    std::cerr << "ERROR: this build's device layer has no colibri_print_instances entry points" << std::endl;
    throw InternalError();
}
int stream_sink(void* user, const uint8_t* p, uint64_t n) {
    std::ostream& o = *static_cast<std::ostream*>(user);
    o.write(reinterpret_cast<const char*>(p), (std::streamsize)n);
    return o.good() ? 0 : 1;
}
// the word table of a class map: every id up to its highest
int upload_words(colibri_ctx* c, const std::unordered_map<unsigned int, std::string>& classes) {
    uint64_t top = 0;
    for (const auto& kv : classes) top = std::max<uint64_t>(top, kv.first);
    const uint64_t        nids = classes.empty() ? 0 : top + 1;
    std::vector<uint64_t> off(1, 0);
    std::vector<uint8_t>  has(1, 0);
    std::string           words;
    if (nids <= (1ull << 26)) {  // (a larger table is refused by colibri_print_classes, with its message)
        std::vector<const std::string*> w(nids, nullptr);
        for (const auto& kv : classes) w[kv.first] = &kv.second;
        off.assign(nids + 1, 0);
        has.assign(nids + 1, 0);
        for (uint64_t k = 0; k < nids; ++k) {
            off[k + 1] = off[k] + (w[k] ? w[k]->size() : 0);
            has[k]     = w[k] != nullptr;
        }
        words.reserve(off[nids]);
        for (uint64_t k = 0; k < nids; ++k)
            if (w[k]) words += *w[k];
    }
    words.push_back('\0');
    return colibri_print_classes(c, off.data(), reinterpret_cast<const uint8_t*>(words.data()), has.data(), nids);
}
// after a print / histogram call: true, or (only under auto, only for a refusal the host path stands in for) false
bool settle(colibri_ctx* c, int rc, const char* what, const char* view, bool loud) {
    if (rc == COLIBRI_ERR_OVERFLOW && !loud) {
        std::cerr << "(" << view << " on the host: " << colibri_last_error(c) << ")" << std::endl;
        return false;
    }
    if (rc != COLIBRI_OK) raise(c, rc, what);
    return true;
}
void fetch_histogram(colibri_ctx* c, uint64_t n, HistogramRows& out) {
    out.counts.assign(n + 1, 0);
    out.patterns.assign(n + 1, 0);
    const int rc = colibri_histogram_fetch(c, out.counts.data(), out.patterns.data());
    if (rc != COLIBRI_OK) raise(c, rc, "colibri_histogram_fetch");
    out.counts.resize(n);
    out.patterns.resize(n);
}
}  // namespace

bool device_print(const std::unordered_map<unsigned int, std::string>& classes, const uint64_t* key_off, const unsigned char* key_bytes, const uint32_t* counts,
                  const uint64_t* ref_off, const uint32_t* ref_sentence, const uint16_t* ref_token, uint64_t npatterns, uint64_t tokens, bool loud, std::ostream& out,
                  bool instantiate, const unsigned char* corpus, uint64_t corpusbytes, uint32_t firstsentence) {
    if (!have_print(loud) || (instantiate && !have_instances(loud))) return false;
    CtxGuard g;
    if (!open_context(g, loud)) return false;
    if (!settle(g.c, upload_words(g.c, classes), "colibri_print_classes", "print", loud)) return false;
    uint64_t nb = 0;
    if (instantiate) {
        int rc = colibri_upload_corpus(g.c, corpus, corpusbytes, firstsentence);
        if (rc == COLIBRI_ERR_CORPUS && !loud) {  // (a corpus the device does not take: the host loop reads it)
            std::cerr << "(print on the host: " << colibri_last_error(g.c) << ")" << std::endl;
            return false;
        }
        if (rc != COLIBRI_OK) raise(g.c, rc, "colibri_upload_corpus");
        rc = colibri_print_instances(g.c, key_off, or_none(key_bytes), counts, ref_off, ref_sentence, ref_token, npatterns, tokens, &stream_sink, &out, &nb);
        return settle(g.c, rc, "colibri_print_instances", "print", loud);
    }
    const int rc = colibri_print_model(g.c, key_off, or_none(key_bytes), counts, ref_off, ref_sentence, ref_token, npatterns, tokens, &stream_sink, &out, &nb);
    return settle(g.c, rc, "colibri_print_model", "print", loud);
}

bool device_print_resident(const std::shared_ptr<void>& device, const TrainResult& model, const std::unordered_map<unsigned int, std::string>& classes, uint64_t tokens, bool loud,
                           std::ostream& out, bool instantiate) {
    if (!have_print(loud) || (instantiate && !have_instances(loud))) return false;
    colibri_ctx* c  = resident_context(device, model);
    uint64_t     nb = 0;
    if (!c) return false;
    if (!settle(c, upload_words(c, classes), "colibri_print_classes", "print", loud)) return false;
    const int rc = instantiate ? colibri_print_instances_resident(c, tokens, &stream_sink, &out, &nb) : colibri_print_model_resident(c, tokens, &stream_sink, &out, &nb);
    if (rc == COLIBRI_ERR_STATE && nb == 0 && out.good()) return false;  // (not a single-device run: the uploaded form)
    return settle(c, rc, instantiate ? "colibri_print_instances_resident" : "colibri_print_model_resident", "print", loud);
}

bool device_histogram(const uint64_t* key_off, const unsigned char* key_bytes, const uint32_t* counts, const uint64_t* ref_off, uint64_t npatterns, int category, uint64_t size,
                      bool loud, HistogramRows& out) {
    if (!have_print(loud)) return false;
    CtxGuard g;
    if (!open_context(g, loud)) return false;
    uint64_t  n  = 0;
    const int rc = colibri_histogram(g.c, key_off, or_none(key_bytes), counts, ref_off, npatterns, category, size, &n);
    if (!settle(g.c, rc, "colibri_histogram", "histogram", loud)) return false;
    fetch_histogram(g.c, n, out);
    return true;
}

bool device_histogram_resident(const std::shared_ptr<void>& device, const TrainResult& model, int category, uint64_t size, bool loud, HistogramRows& out) {
    if (!have_print(loud)) return false;
    colibri_ctx* c = resident_context(device, model);
    uint64_t     n = 0;
    if (!c) return false;
    const int rc = colibri_histogram_resident(c, category, size, &n);
    if (rc == COLIBRI_ERR_STATE) return false;  // (not a single-device run: the uploaded form)
    if (!settle(c, rc, "colibri_histogram_resident", "histogram", loud)) return false;
    fetch_histogram(c, n, out);
    return true;
}

// The reverse-index entry points are referenced weakly, as the print ones are (tests/standin does not implement them).
extern "C" {
int colibri_rindex(colibri_ctx*, const uint64_t*, const uint8_t*, const uint32_t*, uint64_t, uint32_t, int, uint64_t, uint64_t*, uint64_t*) __attribute__((weak));
int colibri_rindex_resident(colibri_ctx*, uint32_t, int, uint64_t, uint64_t*, uint64_t*) __attribute__((weak));
int colibri_rindex_text(colibri_ctx*, colibri_decode_sink, void*, uint64_t*) __attribute__((weak));
}
ReportMode rindex_mode() { return mode_from("COLIBRI_RINDEX"); }
uint64_t   rindex_min_positions() {
    const char*     e = std::getenv("COLIBRI_RINDEX_MIN");
    const long long v = e ? std::atoll(e) : 0;
    return v > 0 ? (uint64_t)v : ~0ull;  // (no measured break-even yet, DESIGN.md §5g: without the variable, auto stays on the host path)
}
namespace {
bool have_rindex(bool loud) {
    if (colibri_print_classes && colibri_rindex && colibri_rindex_resident && colibri_rindex_text) return true;
    if (!loud) return false;
    std::cerr << "ERROR: this build's device layer has no reverse-index entry points" << std::endl;
    throw InternalError();
}
}  // namespace

bool device_rindex_text(const std::unordered_map<unsigned int, std::string>& classes, const uint64_t* key_off, const unsigned char* key_bytes, uint64_t npatterns,
                        const unsigned char* payload, uint64_t nbytes, bool loud, std::ostream& out) {
    if (!have_rindex(loud)) return false;
    CtxGuard g;
    if (!open_context(g, payload, nbytes, loud)) return false;
    if (!settle(g.c, upload_words(g.c, classes), "colibri_print_classes", "reverse index", loud)) return false;
    uint64_t np = 0, nr = 0, nb = 0;
    int      rc = colibri_rindex(g.c, or_none(key_off), or_none(key_bytes), NULL, npatterns, 0, 0, 0, &np, &nr);
    if (!settle(g.c, rc, "colibri_rindex", "reverse index", loud)) return false;
    rc = colibri_rindex_text(g.c, &stream_sink, &out, &nb);
    return settle(g.c, rc, "colibri_rindex_text", "reverse index", loud);
}

bool device_rindex_text_resident(const std::shared_ptr<void>& device, const TrainResult& model, const std::unordered_map<unsigned int, std::string>& classes, bool loud,
                                 std::ostream& out) {
    if (!have_rindex(loud)) return false;
    colibri_ctx* c    = resident_context(device, model);
    uint64_t     npos = 0, nr = 0, nb = 0;
    if (!c) return false;
    if (!settle(c, upload_words(c, classes), "colibri_print_classes", "reverse index", loud)) return false;
    int rc = colibri_rindex_resident(c, 0, 0, 0, &npos, &nr);
    if (rc == COLIBRI_ERR_STATE) return false;  // (not a single-device run: the uploaded form)
    if (!settle(c, rc, "colibri_rindex_resident", "reverse index", loud)) return false;
    rc = colibri_rindex_text(c, &stream_sink, &out, &nb);
    return settle(c, rc, "colibri_rindex_text", "reverse index", loud);
}

// The query entry points are referenced weakly, as the print ones are (tests/standin does not implement them).
extern "C" {
int colibri_query(colibri_ctx*, const uint64_t*, const uint8_t*, const uint32_t*, const uint64_t*, const uint32_t*, const uint16_t*, uint64_t, const uint8_t*, uint64_t, uint32_t,
                  const uint8_t*, int, int, uint64_t*, uint64_t*) __attribute__((weak));
int colibri_query_text(colibri_ctx*, uint64_t, colibri_decode_sink, void*, uint64_t*) __attribute__((weak));
}
ReportMode query_mode() { return mode_from("COLIBRI_QUERY"); }
namespace {
bool have_query(bool loud) {
    if (colibri_print_classes && colibri_query && colibri_query_text) return true;
    if (!loud) return false;
    std::cerr << "ERROR: this build's device layer has no query entry points" << std::endl;
    throw InternalError();
}
}  // namespace

bool device_query(const std::unordered_map<unsigned int, std::string>& classes, const uint64_t* key_off, const unsigned char* key_bytes, const uint32_t* counts, uint64_t npatterns,
                  uint64_t tokens, const std::vector<unsigned char>& payload, const std::vector<unsigned char>& exact, uint32_t first_line, int minlength, int maxlength, bool loud,
                  std::ostream& out) {
    if (!have_query(loud)) return false;
    CtxGuard g;
    if (!open_context(g, loud)) return false;
    if (!settle(g.c, upload_words(g.c, classes), "colibri_print_classes", "query", loud)) return false;
    uint64_t nl = 0, nr = 0, nb = 0;
    int      rc = colibri_query(g.c, or_none(key_off), or_none(key_bytes), or_none(counts), NULL, NULL, NULL, npatterns, or_none(payload.data()), payload.size(), first_line,
                                or_none(exact.data()), minlength, maxlength, &nl, &nr);
    if (!settle(g.c, rc, "colibri_query", "query", loud)) return false;
    rc = colibri_query_text(g.c, tokens, &stream_sink, &out, &nb);
    return settle(g.c, rc, "colibri_query_text", "query", loud);
}

// The subsumption entry points are referenced weakly, as the print ones are (tests/standin does not implement them).
extern "C" {
int colibri_subsume(colibri_ctx*, const uint64_t*, const uint8_t*, uint64_t, int, int, int, uint64_t*) __attribute__((weak));
int colibri_subsume_resident(colibri_ctx*, int, int, int, uint64_t*, uint64_t*) __attribute__((weak));
int colibri_subsume_fetch(colibri_ctx*, uint8_t*, uint64_t*, uint64_t*) __attribute__((weak));
}
ReportMode subsume_mode() { return mode_from("COLIBRI_SUBSUME"); }
uint64_t   subsume_min_patterns() {
    const char*     e = std::getenv("COLIBRI_SUBSUME_MIN");
    const long long v = e ? std::atoll(e) : 0;
    return v > 0 ? (uint64_t)v : 1000000ull;  // (at 1.1 M patterns the device route took 0.42 / 0.28 of the host route's whole train() call)
}
namespace {
bool have_subsume(bool loud) {
    if (colibri_subsume && colibri_subsume_resident && colibri_subsume_fetch) return true;
    if (!loud) return false;
    std::cerr << "ERROR: this build's device layer has no subsumption entry points" << std::endl;
    throw InternalError();
}
void fetch_subsume(colibri_ctx* c, uint64_t np, std::vector<uint8_t>& keep, uint64_t* pruned_non, uint64_t* pruned_sub) {
    keep.assign(np + 1, 0);
    const int rc = colibri_subsume_fetch(c, keep.data(), pruned_non, pruned_sub);
    if (rc != COLIBRI_OK) raise(c, rc, "colibri_subsume_fetch");
    keep.resize(np);
}
}  // namespace

bool device_subsume(const uint64_t* key_off, const unsigned char* key_bytes, uint64_t npatterns, int prunenonsubsumed, int prunesubsumed, int maxlength, bool loud,
                    std::vector<uint8_t>& keep, uint64_t* pruned_non, uint64_t* pruned_sub) {
    if (!have_subsume(loud)) return false;
    CtxGuard g;
    if (!open_context(g, loud)) return false;
    uint64_t  nkept = 0;
    const int rc    = colibri_subsume(g.c, or_none(key_off), or_none(key_bytes), npatterns, prunenonsubsumed, prunesubsumed, maxlength, &nkept);
    if (!settle(g.c, rc, "colibri_subsume", "subsumption prune", loud)) return false;
    fetch_subsume(g.c, npatterns, keep, pruned_non, pruned_sub);
    return true;
}

bool device_subsume_resident(const std::shared_ptr<void>& device, const TrainResult& model, int prunenonsubsumed, int prunesubsumed, int maxlength, bool loud,
                             std::vector<uint8_t>& keep, uint64_t* pruned_non, uint64_t* pruned_sub) {
    if (!have_subsume(loud)) return false;
    colibri_ctx* c  = resident_context(device, model);
    uint64_t     np = 0, nkept = 0;
    if (!c) return false;
    const int rc = colibri_subsume_resident(c, prunenonsubsumed, prunesubsumed, maxlength, &np, &nkept);
    if (rc == COLIBRI_ERR_STATE) return false;  // (not a single-device run: the uploaded form)
    if (!settle(c, rc, "colibri_subsume_resident", "subsumption prune", loud)) return false;
    if (np != model.size()) return false;
    fetch_subsume(c, np, keep, pruned_non, pruned_sub);
    return true;
}

// The recount entry points are referenced weakly, as the print ones are (tests/standin does not implement them).
extern "C" {
int colibri_recount(colibri_ctx*, const uint64_t*, const uint8_t*, uint64_t, int, uint32_t, uint64_t*, uint64_t*) __attribute__((weak));
int colibri_recount_fetch(colibri_ctx*, uint32_t*, uint64_t*, uint32_t*, uint16_t*) __attribute__((weak));
int colibri_recount_info(const colibri_ctx*, uint64_t*, uint64_t*, uint64_t*) __attribute__((weak));
}
ReportMode recount_mode() { return mode_from("COLIBRI_RECOUNT"); }

bool device_recount(const std::shared_ptr<void>& device, const unsigned char* payload, uint64_t nbytes, uint32_t firstsentence, const ConstraintKeys& keys, bool indexed,
                    uint32_t mintokens, TrainResult& out) {
    if (!colibri_recount || !colibri_recount_fetch) {
        std::cerr << "ERROR: this build's device layer has no recount entry points" << std::endl;
        throw InternalError();
    }
    CtxGuard     g;
    colibri_ctx* c = static_cast<colibri_ctx*>(device.get());
    if (c == nullptr) {  // the corpus is not on a device any more: once more
        open_context(g);
        c = g.c;
        const int rc = colibri_upload_corpus(c, payload, nbytes, firstsentence);
        if (rc != COLIBRI_OK) raise(c, rc, "colibri_upload_corpus");
    }
    const uint64_t np = keys.off.empty() ? 0 : keys.off.size() - 1;
    uint64_t       nkept = 0, nrefs = 0;
    int            rc = colibri_recount(c, or_none(keys.off.data()), or_none(keys.bytes.data()), np, indexed ? 1 : 0, mintokens, &nkept, &nrefs);
    if (rc != COLIBRI_OK) raise(c, rc, "colibri_recount");
    out.key_off   = keys.off;
    out.key_bytes = keys.bytes;
    out.counts.assign(np + 1, 0);
    out.ref_off.assign(indexed ? np + 1 : 0, 0);
    out.ref_sentence.assign(nrefs + 1, 0);
    out.ref_token.assign(nrefs + 1, 0);
    rc = colibri_recount_fetch(c, out.counts.data(), indexed ? out.ref_off.data() : NULL, out.ref_sentence.data(), out.ref_token.data());
    if (rc != COLIBRI_OK) raise(c, rc, "colibri_recount_fetch");
    out.counts.resize(np);
    out.device_current = false;
    if (std::getenv("COLIBRI_HOST_TIMING") != nullptr && colibri_recount_info) {
        uint64_t groups = 0, chunks = 0, scratch = 0;
        colibri_recount_info(c, &groups, &chunks, &scratch);
        fprintf(stderr, "COLIBRI_HOST_TIMING recount groups %llu chunks %llu scratch %llu bytes references %llu\n", (unsigned long long)groups, (unsigned long long)chunks,
                (unsigned long long)scratch, (unsigned long long)nrefs);
    }
    return device.get() != nullptr;
}

TrainResult::~TrainResult() {
    if (!ResultPool::on() || key_off.capacity() + key_bytes.capacity() + ref_sentence.capacity() < (1u << 18)) return;  // (small results are not worth keeping)
    ResultPool&                 p = ResultPool::get();
    std::lock_guard<std::mutex> l(p.m);
    if (p.full) return;
    p.key_off.swap(key_off);
    p.key_bytes.swap(key_bytes);
    p.counts.swap(counts);
    p.ref_off.swap(ref_off);
    p.ref_sentence.swap(ref_sentence);
    p.ref_token.swap(ref_token);
    p.full = true;
}

void device_train(const unsigned char* payload, uint64_t nbytes, const colibri_options& opt, uint32_t firstsentence, TrainResult& out, const ConstraintKeys* constraint,
                  bool keep_device, bool continuation, bool as_filter, SeedSet* seed) {
    CtxGuard    g;
    const char* dev = std::getenv("COLIBRI_DEVICE");
    // COLIBRI_HOST_TIMING=1: where a call's wall time goes (context, upload, train, export), one line on stderr
    static const bool timing = std::getenv("COLIBRI_HOST_TIMING") != nullptr;
    typedef std::chrono::steady_clock clk;
    const auto  t0 = clk::now();
    auto        ms = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    const int   device = dev ? std::atoi(dev) : 0;
    const bool  plain  = constraint == NULL && !keep_device;  // (the modes a set of keys switches on stay with a context: such a context is not shared)
    int         rc     = COLIBRI_OK;
    // The idle context of a plain train() keeps its working buffers in HBM (several GB at 10^8 tokens). A run that cannot use it — a constrained / kept-on-device one —
    // would have to find its own memory beside them: it gives the idle context up first. colibri_host::release_cached() does the same on request.
    if (plain) g.c = CtxCache::get().take(device);
    else CtxCache::get().evict(device);
    if (g.c == nullptr) rc = colibri_create(&g.c, device);
    if (rc != COLIBRI_OK) raise(nullptr, rc, "colibri_create");
    const auto t1 = clk::now();
    if ((rc = colibri_upload_corpus(g.c, payload, nbytes, firstsentence)) != COLIBRI_OK) raise(g.c, rc, "colibri_upload_corpus");
    const auto t2 = clk::now();
    if (constraint != NULL && seed != NULL) {  // train() on a loaded model, continued = false: its n-grams and their counts (colibri_set_seed)
        if (colibri_set_seed == nullptr || colibri_seed_fetch == nullptr) {
            std::cerr << "ERROR: the device layer this build is linked against has no colibri_set_seed: expanding a loaded model is not available" << std::endl;
            throw InternalError();
        }
        const uint64_t             np   = constraint->off.empty() ? 0 : constraint->off.size() - 1;
        static const unsigned char none = 0;
        if (np && (rc = colibri_set_seed(g.c, constraint->off.data(), constraint->bytes.empty() ? &none : constraint->bytes.data(), seed->counts.data(), np)) != COLIBRI_OK)
            raise(g.c, rc, "colibri_set_seed");
    } else if (constraint != NULL && as_filter) {
        const uint64_t             np   = constraint->off.empty() ? 0 : constraint->off.size() - 1;
        static const unsigned char none = 0;
        if (np && (rc = colibri_set_filter(g.c, constraint->off.data(), constraint->bytes.empty() ? &none : constraint->bytes.data(), np)) != COLIBRI_OK) raise(g.c, rc, "colibri_set_filter");
    } else if (constraint != NULL && continuation) {
        const uint64_t             np   = constraint->off.empty() ? 0 : constraint->off.size() - 1;
        static const unsigned char none = 0;
        if (np && (rc = colibri_set_continuation(g.c, constraint->off.data(), constraint->bytes.empty() ? &none : constraint->bytes.data(), np)) != COLIBRI_OK)
            raise(g.c, rc, "colibri_set_continuation");
    } else if (constraint != NULL) {
        const uint64_t np = constraint->off.empty() ? 0 : constraint->off.size() - 1;
        if (np == 0) {  // nothing can be a member: the model stays empty, the totals are still the corpus'
            colibri_options plain = opt;
            if (plain.mintokens < 2) plain.mintokens = 2;
            plain.minlength = 1;
            plain.maxlength = 1;
            if ((rc = colibri_train(g.c, &plain, &out.stats)) != COLIBRI_OK) raise(g.c, rc, "colibri_train");
            out.stats.npatterns = 0;
            out.stats.totaltypes = 0;
            out.stats.maxn = out.stats.minn = 0;  // an empty model: nothing of the plain order-1 run that only served the totals stays
            for (int n = 0; n < COLIBRI_MAX_ORDER; ++n) out.stats.found[n] = out.stats.kept[n] = out.stats.pruned[n] = out.stats.admitted[n] = 0;
            out.key_off.assign(1, 0);
            out.key_bytes.assign(1, 0);
            out.counts.clear();
            out.ref_off.assign(1, 0);
            return;
        }
        static const unsigned char none = 0;
        if ((rc = colibri_set_constraint(g.c, constraint->off.data(), constraint->bytes.empty() ? &none : constraint->bytes.data(), np)) != COLIBRI_OK) raise(g.c, rc, "colibri_set_constraint");
    }
    if ((rc = colibri_train(g.c, &opt, &out.stats)) != COLIBRI_OK) raise(g.c, rc, "colibri_train");
    const auto t3 = clk::now();
    uint64_t np = 0, kb = 0, nr = 0;
    if ((rc = colibri_result_sizes(g.c, &np, &kb, &nr)) != COLIBRI_OK) raise(g.c, rc, "colibri_result_sizes");
    const auto t4 = clk::now();
    take_result_buffers(out);  // (arrays of a released model, pages mapped; every element below is written by the export)
    out.key_off.resize(np + 1);
    out.key_bytes.resize(kb + 1);
    out.key_bytes[kb] = 0;
    out.counts.resize(np);
    if (!opt.indexed) {  // (an unindexed result has no reference arrays at all: value_from_result() asks ref_off.empty())
        out.ref_off.clear();
        out.ref_sentence.clear();
        out.ref_token.clear();
    }
    const auto t5 = clk::now();
    struct Report {
        bool on; clk::time_point t0, t1, t2, t3, t4, t5;
        ~Report() {
            if (!on) return;
            auto ms = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
            fprintf(stderr, "COLIBRI_HOST_TIMING create %.2f upload %.2f train %.2f sizes %.2f alloc %.2f export %.2f ms\n", ms(t0, t1), ms(t1, t2), ms(t2, t3), ms(t3, t4), ms(t4, t5),
                    ms(t5, clk::now()));
        }
    } report{timing, t0, t1, t2, t3, t4, t5};
    (void)ms;
    if (opt.indexed) {
        out.ref_off.resize(np + 1);
        out.ref_sentence.resize(nr + 1);
        out.ref_token.resize(nr + 1);
        out.ref_sentence[nr] = 0;
        out.ref_token[nr]    = 0;
        rc = colibri_export_indexed(g.c, out.key_off.data(), out.key_bytes.data(), out.counts.data(), out.ref_off.data(), out.ref_sentence.data(), out.ref_token.data());
        if (rc != COLIBRI_OK) raise(g.c, rc, "colibri_export_indexed");
    } else {
        uint32_t dummy = 0;
        rc = colibri_export_unindexed(g.c, out.key_off.data(), out.key_bytes.data(), np ? out.counts.data() : &dummy);
        if (rc != COLIBRI_OK) raise(g.c, rc, "colibri_export_unindexed");
    }
    if (seed != NULL) {  // what became of the loaded patterns
        seed->row.assign(seed->counts.size(), 0xFFFFFFFFu);
        seed->kept.assign(seed->counts.size(), 1);
        if (!seed->counts.empty() && (rc = colibri_seed_fetch(g.c, seed->row.data(), seed->kept.data())) != COLIBRI_OK) raise(g.c, rc, "colibri_seed_fetch");
    }
    if (keep_device) {  // the caller may follow up on the resident model or corpus (computeflexgrams_fromskipgrams, trainskipgrams_selfconstrained); released with the pending result
        out.device = std::shared_ptr<void>(g.c, [](void* p) { colibri_destroy(static_cast<colibri_ctx*>(p)); });
        g.c        = nullptr;
    }
    if (plain && g.c != nullptr) {  // everything went well: the context waits for the next call
        CtxCache::get().give(device, g.c);
        g.c = nullptr;
    }
}

void release_cached() {
    CtxCache::get().evict(-1);
    if (ResultPool::on()) {
        ResultPool&                 p = ResultPool::get();
        std::lock_guard<std::mutex> l(p.m);
        std::vector<uint64_t>().swap(p.key_off);
        std::vector<unsigned char>().swap(p.key_bytes);
        std::vector<uint32_t>().swap(p.counts);
        std::vector<uint64_t>().swap(p.ref_off);
        std::vector<uint32_t>().swap(p.ref_sentence);
        std::vector<uint16_t>().swap(p.ref_token);
        p.full = false;
    }
}

void device_flexgrams(const std::vector<uint64_t>& key_off, const unsigned char* key_bytes, const std::vector<uint64_t>& ref_off, const uint32_t* ref_sentence,
                      const uint16_t* ref_token, TrainResult& out) {
    CtxGuard g;
    open_context(g);
    const uint64_t np = key_off.empty() ? 0 : key_off.size() - 1;
    uint64_t       nf = 0, kb = 0, nr = 0;
    const int      rc = colibri_flexgrams(g.c, key_off.data(), or_none(key_bytes), ref_off.data(), ref_sentence, ref_token, np, &nf, &kb, &nr);
    if (rc != COLIBRI_OK) raise(g.c, rc, "colibri_flexgrams");
    fetch_flexgrams(g.c, nf, kb, nr, out);
}

// The entry points of the skipgrams of a loaded model are referenced weakly, as the recount ones are (tests/standin does not implement them).
extern "C" {
int colibri_modelskip(colibri_ctx*, const uint64_t*, const uint8_t*, const uint64_t*, const uint32_t*, const uint16_t*, uint64_t, int, int, int, int, int, uint64_t*, uint64_t*, uint64_t*,
                      uint64_t*) __attribute__((weak));
int colibri_modelskip_resident(colibri_ctx*, int, int, int, int, int, uint64_t*, uint64_t*, uint64_t*, uint64_t*) __attribute__((weak));
int colibri_modelskip_fetch(colibri_ctx*, uint64_t*, uint8_t*, uint32_t*, uint32_t*, uint64_t*, uint32_t*, uint16_t*, uint8_t*) __attribute__((weak));
int colibri_modelskip_info(const colibri_ctx*, uint32_t*, uint64_t*, uint64_t*, uint64_t*, uint64_t*, uint64_t*) __attribute__((weak));
}
namespace {
void need_modelskip() {
    if (colibri_modelskip && colibri_modelskip_resident && colibri_modelskip_fetch && colibri_modelskip_info) return;
    std::cerr << "ERROR: this build's device layer has no colibri_modelskip entry points: the skipgrams of a loaded model cannot be computed" << std::endl;
    throw InternalError();
}
void fetch_modelskip(colibri_ctx* c, uint64_t np, uint64_t ns, uint64_t kb, uint64_t nr, SkipgramAnswer& out, SkipgramLog& log) {
    out.key_off.assign(ns + 1, 0);
    out.key_bytes.assign(kb + 1, 0);
    out.counts.assign(ns + 1, 0);
    out.types.assign(ns + 1, 0);
    out.ref_off.assign(ns + 1, 0);
    out.ref_sentence.assign(nr + 1, 0);
    out.ref_token.assign(nr + 1, 0);
    out.keep.assign(np + 1, 1);
    int rc = colibri_modelskip_fetch(c, out.key_off.data(), out.key_bytes.data(), out.counts.data(), out.types.data(), out.ref_off.data(), out.ref_sentence.data(), out.ref_token.data(),
                                     out.keep.data());
    if (rc != COLIBRI_OK) raise(c, rc, "colibri_modelskip_fetch");
    out.counts.resize(ns);
    out.types.resize(ns);
    out.keep.resize(np);
    rc = colibri_modelskip_info(c, &log.orders, log.found, log.pruned, log.extra, NULL, NULL);
    if (rc != COLIBRI_OK) raise(c, rc, "colibri_modelskip_info");
}
}  // namespace

void device_modelskip(const std::vector<uint64_t>& key_off, const unsigned char* key_bytes, const std::vector<uint64_t>& ref_off, const uint32_t* ref_sentence,
                      const uint16_t* ref_token, const colibri_options& o, SkipgramAnswer& out, SkipgramLog& log) {
    need_modelskip();
    CtxGuard g;
    open_context(g);
    const uint64_t np = key_off.empty() ? 0 : key_off.size() - 1;
    uint64_t       ns = 0, kb = 0, nr = 0, gone = 0;
    const int      rc = colibri_modelskip(g.c, key_off.data(), or_none(key_bytes), ref_off.data(), or_none(ref_sentence), or_none(ref_token), np, o.mintokens, o.mintokens_skipgrams,
                                          o.minskiptypes, o.maxlength, o.maxskips, &ns, &kb, &nr, &gone);
    if (rc != COLIBRI_OK) raise(g.c, rc, "colibri_modelskip");
    fetch_modelskip(g.c, np, ns, kb, nr, out, log);
}

bool device_modelskip_resident(const std::shared_ptr<void>& device, const TrainResult& model, const colibri_options& o, SkipgramAnswer& out, SkipgramLog& log) {
    need_modelskip();
    colibri_ctx* c = resident_context(device, model);
    if (!c) return false;
    uint64_t  ns = 0, kb = 0, nr = 0, gone = 0;
    const int rc = colibri_modelskip_resident(c, o.mintokens, o.mintokens_skipgrams, o.minskiptypes, o.maxlength, o.maxskips, &ns, &kb, &nr, &gone);
    if (rc == COLIBRI_ERR_STATE) return false;  // (not a single-device indexed run: the uploaded form)
    if (rc != COLIBRI_OK) raise(c, rc, "colibri_modelskip_resident");
    fetch_modelskip(c, model.size(), ns, kb, nr, out, log);
    return true;
}

void drop_short_patterns(TrainResult& r, int minlength) {
    r.device_current = false;
    const size_t n = r.size();
    const bool   indexed = !r.ref_off.empty();
    size_t       w = 0;
    uint64_t     kb = 0, nr = 0;
    for (size_t j = 0; j < n; ++j) {
        const uint64_t a = r.key_off[j], b = r.key_off[j + 1];
        if ((int)token_count(r.key_bytes.data() + a, (size_t)(b - a)) < minlength) continue;
        std::memmove(r.key_bytes.data() + kb, r.key_bytes.data() + a, (size_t)(b - a));
        r.counts[w]  = r.counts[j];
        if (indexed) {
            const uint64_t ra = r.ref_off[j], rb = r.ref_off[j + 1];
            std::memmove(r.ref_sentence.data() + nr, r.ref_sentence.data() + ra, (size_t)(rb - ra) * sizeof(uint32_t));
            std::memmove(r.ref_token.data() + nr, r.ref_token.data() + ra, (size_t)(rb - ra) * sizeof(uint16_t));
            r.ref_off[w] = nr;
            nr += rb - ra;
        }
        r.key_off[w] = kb;
        kb += b - a;
        ++w;
    }
    r.key_off[w] = kb;
    r.key_off.resize(w + 1);
    r.counts.resize(w);
    if (indexed) {
        r.ref_off[w] = nr;
        r.ref_off.resize(w + 1);
    }
    r.stats.npatterns = w;
}

void print_training_log(const colibri_stats& s, const colibri_options& o, std::ostream& err) {
    if (o.dopatternperline) {  // one pass (reference include/patternmodel.h:1008-1009, :1196-1245)
        err << "Counting patterns from list, one per line" << std::endl;
        if (s.npatterns == 0) {
            err << "None found" << std::endl;
            return;
        }
        err << " Found " << s.npatterns << " ngrams... computing total word types prior to pruning..." << s.totaltypes << "...pruned 0...total kept: " << s.npatterns << std::endl;
        return;
    }
    for (int n = 1; n <= o.maxlength && n < COLIBRI_MAX_ORDER; ++n) {
        err << "Counting " << n << "-grams" << std::endl;
        if (s.found[n] == 0) {
            err << "None found" << std::endl;
            break;
        }
        err << " Found " << s.found[n] << " ngrams...";
        err << "pruned " << s.pruned[n] << "...total kept: " << s.kept[n] << std::endl;
    }
}

// The decoding entry points are referenced weakly, as the comparison ones are.
extern "C" {
int colibri_decode_upload(colibri_ctx*, const uint8_t*, uint64_t, int, uint64_t*) __attribute__((weak));
int colibri_decode_classes(colibri_ctx*, const uint64_t*, const uint8_t*, uint64_t) __attribute__((weak));
int colibri_decode(colibri_ctx*, uint32_t, uint32_t, colibri_decode_sink, void*, uint64_t*, uint64_t*) __attribute__((weak));
}

// a corpus payload (no header) through the device: colibri_decode_upload, the word table of the ids the corpus can reach, colibri_decode
// into `out` in windows of the library's pinned staging
uint64_t device_decode(const std::unordered_map<unsigned int, std::string>& classes, const unsigned char* payload, uint64_t nbytes, int version, unsigned int start,
                       unsigned int end, std::ostream& out) {
    if (!colibri_decode_upload || !colibri_decode_classes || !colibri_decode) {
        std::cerr << "ERROR: this build's device layer has no decoding entry points" << std::endl;
        throw InternalError();
    }
    CtxGuard    g;
    const char* dev    = std::getenv("COLIBRI_DEVICE");
    const int   device = dev ? std::atoi(dev) : 0;
    g.c                = CtxCache::get().take(device);
    int rc             = COLIBRI_OK;
    if (g.c == nullptr) rc = colibri_create(&g.c, device);
    if (rc != COLIBRI_OK) raise(nullptr, rc, "colibri_create");
    static const unsigned char none = 0;
    uint64_t                   maxclass = 0;
    if ((rc = colibri_decode_upload(g.c, nbytes ? payload : &none, nbytes, version, &maxclass)) != COLIBRI_OK) raise(g.c, rc, "colibri_decode_upload");
    // the table covers the ids up to the lower of the corpus' highest id and the class map's: no id above either has a word to print
    uint64_t top = 0;
    for (const auto& kv : classes) top = std::max<uint64_t>(top, kv.first);
    const uint64_t        nids = std::min(top, maxclass) + 1;
    std::vector<uint64_t> off;
    std::string           words;
    if (nids <= (1ull << 26)) {  // (a larger table is refused by colibri_decode_classes, with its message)
        std::vector<const std::string*> w(nids, nullptr);
        for (const auto& kv : classes)
            if (kv.first < nids) w[kv.first] = &kv.second;
        off.assign(nids + 1, 0);
        for (uint64_t k = 0; k < nids; ++k) off[k + 1] = off[k] + (w[k] ? w[k]->size() : 0);
        words.reserve(off[nids]);
        for (uint64_t k = 0; k < nids; ++k)
            if (w[k]) words += *w[k];
    } else {
        off.assign(nids + 1, 0);  // (only its size is looked at before the refusal)
    }
    if ((rc = colibri_decode_classes(g.c, off.data(), reinterpret_cast<const uint8_t*>(words.data()), nids)) != COLIBRI_OK) raise(g.c, rc, "colibri_decode_classes");
    struct Sink {
        static int write(void* user, const uint8_t* p, uint64_t n) {
            std::ostream& o = *static_cast<std::ostream*>(user);
            o.write(reinterpret_cast<const char*>(p), (std::streamsize)n);
            return o.good() ? 0 : 1;
        }
    };
    uint64_t outbytes = 0, nlines = 0;
    if ((rc = colibri_decode(g.c, start, end, &Sink::write, &out, &outbytes, &nlines)) != COLIBRI_OK) raise(g.c, rc, "colibri_decode");
    CtxCache::get().give(device, g.c);
    g.c = nullptr;
    return nlines;
}

// The n-gram extraction entry points are referenced weakly, as the decoding ones are (tests/standin does not implement them).
extern "C" {
int colibri_ngrams(colibri_ctx*, uint32_t, colibri_decode_sink, void*, uint64_t*, uint64_t*) __attribute__((weak));
int colibri_ngrams_info(const colibri_ctx*, uint64_t*, uint64_t*, uint64_t*) __attribute__((weak));
}

// colibri-extractngrams (csrc/ngrams.hpp): per data file colibri_decode_upload of the payload behind the A2 02 signature and colibri_ngrams into
// `out` in the library's windows; the class map goes up once, as the word table of colibri_print_classes, before the first file that has data
uint64_t extract_ngrams(const ClassDecoder& classdecoder, const std::vector<std::string>& datafiles, int n, std::ostream& out) {
    if (n < 1) {
        std::cerr << "ERROR: the n-gram size must be at least 1 (got " << n << ")" << std::endl;
        throw InternalError();
    }
    CtxGuard    g;
    const char* dev    = std::getenv("COLIBRI_DEVICE");
    const int   device = dev ? std::atoi(dev) : 0;
    uint64_t    rows   = 0;
    for (const std::string& datafile : datafiles) {
        std::ifstream in(datafile, std::ios::in | std::ios::binary);
        if (!in.good()) (void)getdataversion(in);  // (its message for a file that cannot be opened, InternalError)
        in.seekg(0, std::ios::end);
        const uint64_t size = (uint64_t)in.tellg();
        if (size == 0) continue;  // (the reference ends in an uncaught exception)
        if (getdataversion(in) != 2) {  // (its message and InternalError for plain text; leaves the stream behind the signature of version 2 data)
            std::cerr << "ERROR: Supplied data file is not version 2 Colibri data (it has no A2 02 signature, or is version 1 data); n-grams are extracted from version 2 data only..."
                      << std::endl;
            throw InternalError();
        }
        if (size - 2 >= 0xFFFFFF00ull) {  // (ingest's limit and message, before the file is read)
            std::cerr << "ERROR: corpus shard of " << size - 2 << " bytes exceeds the 4 GiB per-device limit (32-bit byte offsets); shard it" << std::endl;
            throw InternalError();
        }
        if (!colibri_decode_upload || !colibri_print_classes || !colibri_ngrams || !colibri_ngrams_info) {
            std::cerr << "ERROR: this build's device layer has no n-gram extraction entry points" << std::endl;
            throw InternalError();
        }
        in.clear();
        const std::vector<unsigned char> raw((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
        int rc = COLIBRI_OK;
        if (g.c == nullptr) {
            g.c = CtxCache::get().take(device);
            if (g.c == nullptr) rc = colibri_create(&g.c, device);
            if (rc != COLIBRI_OK) raise(nullptr, rc, "colibri_create");
            if ((rc = upload_words(g.c, classdecoder.words())) != COLIBRI_OK) raise(g.c, rc, "colibri_print_classes");
        }
        static const unsigned char none = 0;
        if ((rc = colibri_decode_upload(g.c, raw.empty() ? &none : raw.data(), raw.size(), 2, nullptr)) != COLIBRI_OK) raise(g.c, rc, "colibri_decode_upload");
        uint64_t outbytes = 0, r = 0;
        if ((rc = colibri_ngrams(g.c, (uint32_t)n, &stream_sink, &out, &outbytes, &r)) != COLIBRI_OK) raise(g.c, rc, "colibri_ngrams");
        rows += r;
    }
    if (g.c) CtxCache::get().give(device, g.c);
    g.c = nullptr;
    return rows;
}
uint64_t extract_ngrams(const ClassDecoder& classdecoder, const std::string& datafile, int n, std::ostream& out) {
    return extract_ngrams(classdecoder, std::vector<std::string>{datafile}, n, out);
}

}  // namespace colibri_host

int getmodeltype(const std::string& filename) {
    std::ifstream in(filename, std::ios::in | std::ios::binary);
    unsigned char null = 1, type = 0;
    in.read((char*)&null, 1);
    in.read((char*)&type, 1);
    return (in.good() && null == 0) ? (int)type : 0;
}

// ---------------------------------------------------------------------------------------------------
// IndexedCorpus
// ---------------------------------------------------------------------------------------------------
void IndexedCorpus::load(std::istream& in, bool) {
    std::vector<unsigned char> payload = colibri_host::read_corpus_payload(in);
    delete[] corpus;
    corpussize = payload.size();
    corpus     = new unsigned char[corpussize + 16];
    std::memset(corpus, 0, corpussize + 16);
    if (corpussize) std::memcpy(corpus, payload.data(), corpussize);
    sentencestart.clear();
    delimiters         = 0;
    bool prevdelimiter = true, prevhigh = false;
    for (size_t i = 0; i < corpussize; ++i) {  // every delimiter opens a new sentence, empty ones included (reference src/pattern.cpp:1947-1958)
        if (prevdelimiter) {
            sentencestart.push_back(i);
            prevdelimiter = false;
        }
        if (!prevhigh && corpus[i] == 0) {
            prevdelimiter = true;
            ++delimiters;
        }
        prevhigh = corpus[i] >= 128;
    }
}
void IndexedCorpus::load(const std::string& filename, bool debug) {
    std::ifstream in(filename, std::ios::in | std::ios::binary);
    if (!in.good()) {
        std::cerr << "ERROR: Unable to load file " << filename << std::endl;
        throw InternalError();
    }
    load(in, debug);
}
PatternPointer IndexedCorpus::getsentence(int sentence) const {
    if (sentence < 1 || (size_t)sentence > sentencestart.size()) throw KeyError();
    const size_t b = sentencestart[sentence - 1];
    size_t       e = b;
    bool         prevhigh = false;
    while (e < corpussize && (prevhigh || corpus[e] != 0)) {
        prevhigh = corpus[e] >= 128;
        ++e;
    }
    return PatternPointer(corpus + b, e - b);
}
PatternPointer IndexedCorpus::getpattern(const IndexReference& begin, int length) const {
    const PatternPointer s = getsentence((int)begin.sentence);
    size_t               tok = 0, i = 0, startb = 0;
    bool                 found = begin.token == 0;
    for (; i < s.bytes && !found; ++i) {
        if (s.data[i] < 128) {
            ++tok;
            if (tok == begin.token) {
                startb = i + 1;
                found  = true;
            }
        }
    }
    if (!found) throw KeyError();
    size_t e = startb;
    int    got = 0;
    while (e < s.bytes && got < length) {
        if (s.data[e] < 128) ++got;
        ++e;
    }
    if (got < length) throw KeyError();
    return PatternPointer(s.data + startb, e - startb);
}
bool IndexedCorpus::instancewindow(uint32_t first_sentence, uint32_t sentence, uint32_t token, uint32_t n, PatternPointer& window) const {
    const colibri_host::InstanceWindow w = colibri_host::instance_window(corpus, corpussize, sentencestart.data(), sentencestart.size(), first_sentence, sentence, token, n);
    if (!w.fits) return false;
    window = PatternPointer(corpus + w.begin, w.bytes);
    return true;
}
PatternPointer IndexedCorpus::findpattern(const IndexReference& begin, const Pattern& pattern, PatternCategory resultcategory) const {
    const PatternCategory cat = pattern.category();
    if (cat == FLEXGRAM) {
        std::cerr << "ERROR: IndexedCorpus::findpattern: flexgram patterns are not instantiated (the reference's walk accepts gaps of exactly one token, DESIGN.md §6)" << std::endl;
        throw InternalError();
    }
    PatternPointer window = getpattern(begin, (int)pattern.n());  // KeyError outside the sentence
    // token by token: a gap of the skipgram (the one-byte token 03) stands for whatever the corpus holds there, every other token must be the corpus' own
    const unsigned char *p = pattern.data, *w = window.data;
    const size_t         pbytes = pattern.bytesize();
    uint32_t             mask = 0;
    for (size_t i = 0, j = 0, t = 0; i < pbytes; ++t) {
        size_t pl = 1, wl = 1;
        while (p[i + pl - 1] >= 128) ++pl;
        while (w[j + wl - 1] >= 128) ++wl;
        if (cat == SKIPGRAM && pl == 1 && p[i] == 3) {
            mask |= bitmask_of((int)t);
        } else if (pl != wl || std::memcmp(p + i, w + j, pl) != 0) {
            throw KeyError();
        }
        i += pl;
        j += wl;
    }
    if (cat == NGRAM || resultcategory == NGRAM) return window;
    window.mask = mask | (resultcategory == FLEXGRAM ? 1u << 31 : 0u);
    return window;
}

// ---------------------------------------------------------------------------------------------------
// ClassDecoder: decoding (reference src/classdecoder.cpp:132-257)
// ---------------------------------------------------------------------------------------------------
std::vector<std::string> ClassDecoder::decodeseq(const std::vector<int>& seq) {
    std::vector<std::string> result;
    for (const int c : seq) result.push_back(classes[(unsigned int)c]);
    return result;
}

void ClassDecoder::decodepayload(const unsigned char* payload, uint64_t nbytes, int version, std::ostream& out, unsigned int start, unsigned int end, bool quiet) const {
    const uint64_t nlines = colibri_host::device_decode(classes, payload, nbytes, version, start, end, out);
    if (!quiet) std::cerr << "Processed " << nlines << " lines" << std::endl;
}

void ClassDecoder::decodefile(const std::string& filename, std::ostream& out, unsigned int start, unsigned int end, bool quiet) {
    std::ifstream       in(filename, std::ios::in | std::ios::binary);
    const unsigned char version = getdataversion(in);  // (its messages and InternalError for a missing or plain-text file)
    if (version == 1) {
        decodefile_v1(in, out, start, end, quiet);
        return;
    }
    in.clear();
    const std::vector<unsigned char> raw((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    decodepayload(raw.data(), raw.size(), 2, out, start, end, quiet);
}

void ClassDecoder::decodefile_v1(std::ifstream& in, std::ostream& out, unsigned int start, unsigned int end, bool quiet) {
    in.clear();
    const std::vector<unsigned char> raw((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    in.close();
    decodepayload(raw.data(), raw.size(), 1, out, start, end, quiet);
}

std::string ClassDecoder::decodefiletostring(const std::string& filename, unsigned int start, unsigned int end, bool quiet) {
    std::ostringstream ss;
    decodefile(filename, ss, start, end, quiet);
    return ss.str();
}

void ClassDecoder::add(const unsigned int cls, const std::string& word) {
    classes[cls] = word;
    if (cls > highestclass) highestclass = cls;
}

void ClassDecoder::prune(unsigned int threshold) {
    for (unsigned int i = threshold; i <= highestclass; ++i) {
        classes.erase(i);
        if (i == 0xFFFFFFFFu) break;
    }
    highestclass = threshold - 1;
}

// ---- ClassEncoder: what needs no device (the class file, one line of text into key bytes; reference src/classencoder.cpp:83-132, :369-447). The corpus-proportional
// calls are in classencoder.cpp, over the device library. ----
ClassEncoder::ClassEncoder(const unsigned int minlength_, const unsigned int maxlength_) : highestclass(5), minlength(minlength_), maxlength(maxlength_) {}
ClassEncoder::ClassEncoder(const std::string& filename, const unsigned int minlength_, const unsigned int maxlength_) { load(filename, minlength_, maxlength_); }

void ClassEncoder::load(const std::string& filename, const unsigned int minlength_, const unsigned int maxlength_) {
    highestclass = 0;
    minlength    = minlength_;
    maxlength    = maxlength_;
    if (minlength || maxlength) {
        std::cerr << "ERROR: word length limits are not on the MI355X-accelerated path" << std::endl;
        throw InternalError();
    }
    std::ifstream IN(filename);
    if (!IN) {
        std::cerr << "ERROR: File does not exist: " << filename << std::endl;
        throw InternalError();
    }
    while (IN.good()) {
        std::string line;
        std::getline(IN, line);
        const size_t tab = line.find('\t');
        if (tab == std::string::npos) continue;
        const unsigned int cls    = (unsigned int)std::atoi(line.substr(0, tab).c_str());
        classes[line.substr(tab + 1)] = cls;
        if (cls > highestclass) highestclass = cls;
    }
    classes["{?}"]  = unknownclass;
    classes["{*}"]  = skipclass;
    classes["{**}"] = flexclass;
    classes["{|}"]  = boundaryclass;
}

namespace {
// the class as little-endian base-128 digits, the high bit on every byte but the last (reference src/classencoder.cpp:22-42)
unsigned int class_to_bytes(unsigned char* out, unsigned int cls) {
    unsigned int n = 0;
    do {
        const unsigned char b = (unsigned char)(cls & 127u);
        cls >>= 7;
        out[n++] = cls ? (unsigned char)(b | 128u) : b;
    } while (cls);
    return n;
}
std::string trim_word(const std::string& s) {
    const char*  blanks = " \t\n\r\b";
    const size_t a      = s.find_first_not_of(blanks);
    if (a == std::string::npos) return std::string();
    return s.substr(a, s.find_last_not_of(blanks) - a + 1);
}
}  // namespace

int ClassEncoder::encodestring(const std::string& line, unsigned char* outputbuffer, bool allowunknown, bool autoaddunknown, unsigned int* nroftokens) {
    int       outputcursor = 0, start = 0;
    const int l = (int)line.length();
    for (int i = 0; i < l; i++) {
        if (line[i] != ' ' && i != l - 1) continue;
        const std::string word = trim_word(std::string(line.begin() + start, line.begin() + (line[i] == ' ' ? i : i + 1)));
        start                  = i + 1;
        if (word.empty()) continue;
        unsigned int cls = 0, repeat = 1;
        if (word == "{*}") {
            cls = skipclass;
        } else if (word == "{**}") {
            cls = flexclass;
        } else if (word == "{?}") {
            cls = unknownclass;
        } else if (word.substr(0, 2) == "{*" && word.substr(word.size() - 2, 2) == "*}") {
            const int n = std::atoi(word.substr(2, word.size() - 4).c_str());
            cls         = skipclass;
            repeat      = n > 0 ? (unsigned int)n : 0u;
        } else {
            auto it = classes.find(word);
            if (it != classes.end()) {
                cls = it->second;
            } else if (autoaddunknown) {
                cls           = ++highestclass;
                classes[word] = cls;
            } else if (!allowunknown) {
                throw UnknownTokenError();
            } else {
                cls = unknownclass;
            }
        }
        for (unsigned int j = 0; j < repeat; ++j) {
            outputcursor += (int)class_to_bytes(outputbuffer + outputcursor, cls);
            if (nroftokens != NULL) (*nroftokens)++;
        }
    }
    return outputcursor;
}

Pattern ClassEncoder::buildpattern(const std::string& patternstring, bool allowunknown, bool autoaddunknown) {
    std::vector<unsigned char> buffer(5 * patternstring.size() + 8);  // (a word of one byte becomes at most five bytes; {*N*} is bounded below)
    // {*N*} writes N bytes for a word of at least five: count what the line needs before writing
    size_t need = buffer.size();
    for (size_t a = patternstring.find("{*"); a != std::string::npos; a = patternstring.find("{*", a + 2)) {
        const int n = std::atoi(patternstring.c_str() + a + 2);
        if (n > 0) need += (size_t)n;
    }
    buffer.resize(need);
    const int size = encodestring(patternstring, buffer.data(), allowunknown, autoaddunknown);
    return Pattern(buffer.data(), (size_t)size);
}
