// patternmodel.h — PatternModelOptions / PatternModel<uint32_t> / IndexedPatternModel<> : the C++ face of the
// MI355X-native pattern-model builder. Same class names, method names, argument orders and error behaviour as the
// reference (include/patternmodel.h:103-213 options, :546-2674 PatternModel, :2682-3875 IndexedPatternModel) so that
// callers such as src/patternmodeller.cpp:316-319 or src/benchmarks.cpp:228-237 compile against it unchanged; what
// train() does is different: the corpus goes to HBM and the whole informed-iterative counting (reference :880-1345)
// runs in libcolibri_hip.so through the C ABI of include/colibri_hip.h. There is no host implementation of the
// counting loop: options outside the accelerated subset raise InternalError after a message on stderr, exactly as the
// reference reports its own errors (include/common.h:41-44).
#ifndef COLIBRI_AMD_PATTERNMODEL_H
#define COLIBRI_AMD_PATTERNMODEL_H
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <algorithm>
#include <fstream>
#include <iomanip>
#include <iostream>
#include <limits>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <sstream>
#include <string>
#include <unordered_set>
#include <vector>
#include <cstring>
#include <thread>

#include "classencoder.h"
#include "colibri_hip.h"
#include "expand_merge.h"
#include "keep_rows.h"
#include "skipgram_merge.h"
#include "patternstore.h"

enum ModelType {
    UNINDEXEDPATTERNMODEL        = 10,
    UNINDEXEDPATTERNPOINTERMODEL = 11,
    INDEXEDPATTERNMODEL          = 20,
    INDEXEDPATTERNPOINTERMODEL   = 21,
    PATTERNSETMODEL              = 30,
    PATTERNALIGNMENTMODEL        = 40,
};

/** reads the type byte of a model file (reference src/patternmodel.cpp:3-15) */
int getmodeltype(const std::string& filename);

class NoSuchPattern : public std::exception {
    const char* what() const throw() override { return "Pattern not found in model"; }
};

/** Options for training / loading — public fields and defaults of reference include/patternmodel.h:103-180. */
class PatternModelOptions {
  public:
    int  MINTOKENS, MINTOKENS_SKIPGRAMS, MINTOKENS_UNIGRAMS, MINLENGTH, MAXLENGTH, MAXBACKOFFLENGTH;
    bool DOSKIPGRAMS, DOSKIPGRAMS_EXHAUSTIVE;
    int  MINSKIPTYPES, MAXSKIPS;
    bool DOREVERSEINDEX, DOPATTERNPERLINE;
    int  PRUNENONSUBSUMED, PRUNESUBSUMED;
    bool DOREMOVEINDEX, DOREMOVENGRAMS, DOREMOVESKIPGRAMS, DOREMOVEFLEXGRAMS, DORESET;
    bool QUIET, DEBUG;
    PatternModelOptions()
        : MINTOKENS(-1), MINTOKENS_SKIPGRAMS(-1), MINTOKENS_UNIGRAMS(1), MINLENGTH(1), MAXLENGTH(100), MAXBACKOFFLENGTH(100), DOSKIPGRAMS(false),
          DOSKIPGRAMS_EXHAUSTIVE(false), MINSKIPTYPES(2), MAXSKIPS(3), DOREVERSEINDEX(true), DOPATTERNPERLINE(false), PRUNENONSUBSUMED(0), PRUNESUBSUMED(0),
          DOREMOVEINDEX(false), DOREMOVENGRAMS(false), DOREMOVESKIPGRAMS(false), DOREMOVEFLEXGRAMS(false), DORESET(false), QUIET(false), DEBUG(false) {}
};

/** The limited polymorphic view other components take of a model (reference include/patternmodel.h:234-287). */
class PatternModelInterface {
  public:
    virtual ~PatternModelInterface() {}
    virtual int          getmodeltype() const                       = 0;
    virtual int          getmodelversion() const                    = 0;
    virtual bool         has(const Pattern&) const                  = 0;
    virtual bool         has(const PatternPointer&) const           = 0;
    virtual size_t       size() const                               = 0;
    virtual unsigned int occurrencecount(const Pattern& pattern)    = 0;
    virtual double       frequency(const Pattern&)                  = 0;
    virtual int          maxlength() const                          = 0;
    virtual int          minlength() const                          = 0;
    virtual unsigned int types()                                    = 0;
    virtual unsigned int tokens() const                             = 0;
    /** (this build) the keys of all patterns, for installing the model as a device-side constraint set; false = cannot enumerate */
    virtual bool collect_keys(std::vector<uint64_t>&, std::vector<unsigned char>&) { return false; }
};

namespace colibri_host {

/** flat result of one device training run, as exported through colibri_export_* */
struct TrainResult {
    colibri_stats              stats{};
    std::vector<uint64_t>      key_off;
    std::vector<unsigned char> key_bytes;
    std::vector<uint32_t>      counts;
    std::vector<uint64_t>      ref_off;
    std::vector<uint32_t>      ref_sentence;
    std::vector<uint16_t>      ref_token;
    std::shared_ptr<void>      device;  ///< (optional) the device context that still holds this model in HBM, for follow-up passes that need no host round trip
    bool                       device_current = true;  ///< the arrays are still what `device` holds (cleared by every host-side edit of them)
    size_t                     size() const { return counts.size(); }
    TrainResult()                              = default;
    TrainResult(const TrainResult&)            = default;
    TrainResult(TrainResult&&)                 = default;
    TrainResult& operator=(const TrainResult&) = default;
    TrainResult& operator=(TrainResult&&)      = default;
    ~TrainResult();  ///< the arrays go back to the process' result pool (colibri_host.cpp): the next export writes into pages that are already mapped
};

/** MINLENGTH > 1 in an unconstrained run: the reference counts the shorter orders (the look-back needs them) and prunes them away afterwards
 *  (patternmodel.h:1221-1230, :1339-1343), so the model is the full one without its patterns of fewer than `minlength` tokens */
void drop_short_patterns(TrainResult& r, int minlength);
/** the patterns whose flag is set, in place and in order (keep_rows.h: one linear pass over the key, count and reference arrays); the arrays are no
 *  longer what the device holds */
inline void keep_patterns(TrainResult& r, const uint8_t* keep) {
    r.device_current  = false;
    r.stats.npatterns = keep_rows(r.key_off, r.key_bytes, r.counts, r.ref_off, r.ref_sentence, r.ref_token, keep);
}
/** whole corpus file -> v2 payload (header stripped; v1 data converted, reference src/classencoder.cpp:602-647) */
std::vector<unsigned char> read_corpus_payload(std::istream& in);
/** the keys a run is constrained to (colibri_set_constraint), or NULL */
struct ConstraintKeys {
    std::vector<uint64_t>      off;
    std::vector<unsigned char> bytes;
};
/** the model a run expands (colibri_set_seed): the count of every key of the ConstraintKeys passed with it, and after the run, per key, the result row that
 *  carries it (0xFFFFFFFF: none) and whether it stays in the model (colibri_seed_fetch) */
struct SeedSet {
    std::vector<uint32_t> counts, row;
    std::vector<uint8_t>  kept;
};
/** upload + train + export through the C ABI; prints the library's message on stderr and throws InternalError on any status != 0 */
void device_train(const unsigned char* payload, uint64_t nbytes, const colibri_options& opt, uint32_t firstsentence, TrainResult& out, const ConstraintKeys* constraint = NULL,
                  bool keep_device = false, bool continuation = false /* the keys are the model a continued run starts from (colibri_set_continuation) */,
                  bool as_filter = false /* the keys are train()'s filter (colibri_set_filter) */, SeedSet* seed = NULL /* the keys are the model the run expands */);
/** the same across `world` GPUs of this node (src/sharded.cpp): the corpus cut into contiguous sentence ranges, one device context and host thread per rank,
 *  RCCL for the exchange of candidate counts; the result is the union of the ranks' exports. Not for constrained runs and pattern lists. */
void device_train_sharded(const unsigned char* payload, uint64_t nbytes, const colibri_options& opt, uint32_t firstsentence, TrainResult& out, int world);
/** what the library keeps between plain train() calls of a process — the idle device context of every GPU (its working buffers stay reserved in HBM) and the arrays of the
 * last released model — given back now (a long-lived caller that is done training, or one that shares the GPU with other work) */
void release_cached();
/** how many GPUs train() uses: set_gpus(n) (the CLI's --gpus), else the environment's COLIBRI_GPUS, else 1 */
void set_gpus(int n);
int  gpus();
/** flexgrams abstracted from the skipgrams of an indexed model given in export layout (colibri_flexgrams + colibri_flexgrams_fetch) */
void device_flexgrams(const std::vector<uint64_t>& key_off, const unsigned char* key_bytes, const std::vector<uint64_t>& ref_off, const uint32_t* ref_sentence,
                      const uint16_t* ref_token, TrainResult& out);
/** the same on the model a device_train(..., keep_device = true) left resident (colibri_flexgrams_resident) */
void device_flexgrams_resident(const std::shared_ptr<void>& device, TrainResult& out);
/** rows of a co-occurrence table in output order (value descending, then A's key bytes, then B's): pattern numbers into the model's flat arrays */
struct CoocRows {
    std::vector<uint32_t> a, b, count;
    std::vector<double>   value;
};
/** sentence co-occurrence of an indexed model given in export layout, with the corpus payload as its reverse index (colibri_cooc + colibri_cooc_fetch);
 *  mode COLIBRI_COOC_COUNT (threshold) or COLIBRI_COOC_NPMI (npmi_threshold) */
void device_cooc(const std::vector<uint64_t>& key_off, const unsigned char* key_bytes, const std::vector<uint64_t>& ref_off, const uint32_t* ref_sentence, const uint16_t* ref_token,
                 const unsigned char* payload, uint64_t nbytes, uint32_t threshold, int mode, double npmi_threshold, CoocRows& out);
/** the same on the model a device_train(..., keep_device = true) left resident (colibri_cooc_resident); false (nothing done) when `model` no longer
 *  holds what the device holds */
bool device_cooc_resident(const std::shared_ptr<void>& device, const TrainResult& model, uint32_t threshold, int mode, double npmi_threshold, CoocRows& out);
/** rows of a relation table in output order (A's pattern number, then count descending, then B's key bytes): pattern numbers into the model's flat arrays */
struct RelationRows {
    std::vector<uint32_t> a, b, count;
};
/** one relation (COLIBRI_REL_*) of every pattern of an indexed model given in export layout, with the corpus payload as its reverse index
 *  (colibri_relations + colibri_relations_fetch) */
void device_relations(const std::vector<uint64_t>& key_off, const unsigned char* key_bytes, const std::vector<uint64_t>& ref_off, const uint32_t* ref_sentence,
                      const uint16_t* ref_token, const unsigned char* payload, uint64_t nbytes, int kind, uint32_t threshold, RelationRows& out);
/** the same on the model a device_train(..., keep_device = true) left resident (colibri_relations_resident); false (nothing done) when `model` no
 *  longer holds what the device holds */
bool device_relations_resident(const std::shared_ptr<void>& device, const TrainResult& model, int kind, uint32_t threshold, RelationRows& out);
/** rows of the skip-content table in output order (A's pattern number, then count descending, then the content's bytes): b = the content's pattern
 *  number in the model or 0xFFFFFFFF, content i = bytes [content_off[i], content_off[i + 1]) */
struct SkipContentRows {
    std::vector<uint32_t>      a, b, count;
    std::vector<uint64_t>      content_off;
    std::vector<unsigned char> content_bytes;
};
/** the skip content of every skipgram of an indexed model given in export layout, sliced from the corpus payload (colibri_skipcontent + _fetch) */
void device_skipcontent(const std::vector<uint64_t>& key_off, const unsigned char* key_bytes, const std::vector<uint64_t>& ref_off, const uint32_t* ref_sentence,
                        const uint16_t* ref_token, const unsigned char* payload, uint64_t nbytes, SkipContentRows& out);
/** the same on the model a device_train(..., keep_device = true) left resident (colibri_skipcontent_resident); false (nothing done) when `model` no
 *  longer holds what the device holds */
bool device_skipcontent_resident(const std::shared_ptr<void>& device, const TrainResult& model, SkipContentRows& out);
/** rows of a model comparison in output order (colibri_compare + colibri_compare_fetch): a representative occurrence of each row (model, index into that model's
 *  input arrays), its log-likelihood, and nrows x nmodels counts / (category, size) group totals (unsigned int, as totaloccurrencesingroup returns them) */
struct CompareRows {
    size_t                nmodels = 0;
    std::vector<uint32_t> model, index, observed, group_totals;
    std::vector<double>   ll;
};
/** one model of a comparison, in export layout: key offsets (npatterns + 1), key bytes, counts, tokens() */
struct CompareInput {
    const uint64_t*      key_off   = NULL;
    const unsigned char* key_bytes = NULL;
    const uint32_t*      counts    = NULL;
    uint64_t             npatterns = 0;
    uint64_t             tokens    = 0;
};
/** the log-likelihood comparison of N >= 2 models in one device call: rows ordered by ll descending, then key bytes (sorted = false: by first occurrence) */
void device_compare(const std::vector<CompareInput>& models, bool conjunctiononly, bool sorted, CompareRows& out);
/** which path computestats() / computecoveragestats() take (environment COLIBRI_REPORT = host | device | auto): auto takes the device for a model of
 *  at least report_min_work() patterns + references when one is usable, and the host path otherwise; device fails loudly instead of falling back */
enum ReportMode { REPORT_AUTO = 0, REPORT_HOST = 1, REPORT_DEVICE = 2 };
ReportMode report_mode();
/** the size from which auto goes to the device (environment COLIBRI_REPORT_MIN overrides it) */
uint64_t report_min_work();
/** the plain per-group values of colibri_coverage: 4 * G entries each, group (category, size) at category * G + size, 0 = all */
struct CoverageGroups {
    uint32_t              G = 0;
    std::vector<uint64_t> patterns, counts, types, tokens;
};
/** the coverage report of a model in export layout (colibri_coverage + colibri_coverage_fetch); counts NULL: a pattern's count is its number of references,
 *  ref_* NULL: unindexed; tokens = false: no covered tokens (computestats). false = the host path has to do it: no device layer or device, or the
 *  call was refused for its scratch budget — unless `loud`, which turns each of those into an error */
bool device_coverage(const uint64_t* key_off, const unsigned char* key_bytes, const uint32_t* counts, const uint64_t* ref_off, const uint32_t* ref_sentence, const uint16_t* ref_token,
                     uint64_t npatterns, bool tokens, bool loud, CoverageGroups& out);
/** the same on the model a device_train(..., keep_device = true) left resident (colibri_coverage_resident); false also when `model` no longer holds what
 *  the device holds */
bool device_coverage_resident(const std::shared_ptr<void>& device, const TrainResult& model, bool tokens, bool loud, CoverageGroups& out);
/** which path print() / histogram() take (environment COLIBRI_PRINT / COLIBRI_HISTOGRAM = host | device | auto, with COLIBRI_REPORT's semantics): auto
 *  takes the device for a model of at least print_min_work() patterns + references when one is usable; device fails loudly instead of falling back */
ReportMode print_mode();
ReportMode histogram_mode();
/** the size from which auto goes to the device: environment COLIBRI_PRINT_MIN; unset, auto stays on the host path (no break-even has been measured) */
uint64_t print_min_work();
/** is `out` in the state the device-side rows are written for: precision 6, no fixed / scientific / showpoint / uppercase / showpos, width 0 */
bool stream_in_default_float_state(const std::ostream& out);
/** the rows of print() for a model in export layout, written to `out` (colibri_print_classes + colibri_print_model; counts NULL: a pattern's count is its
 *  number of references, ref_* NULL: unindexed). false = the host path has to do it (nothing was written): no device layer or device, or the call was
 *  refused for its size — unless `loud`, which turns each of those into an error. instantiate: the rows of print(..., instantiate = true) for an indexed model
 *  (colibri_print_instances): `corpus` (numbered from firstsentence) is uploaded first, and the resident form below reads the corpus its context holds */
bool device_print(const std::unordered_map<unsigned int, std::string>& classes, const uint64_t* key_off, const unsigned char* key_bytes, const uint32_t* counts,
                  const uint64_t* ref_off, const uint32_t* ref_sentence, const uint16_t* ref_token, uint64_t npatterns, uint64_t tokens, bool loud, std::ostream& out,
                  bool instantiate = false, const unsigned char* corpus = NULL, uint64_t corpusbytes = 0, uint32_t firstsentence = 1);
/** the same on the model a device_train(..., keep_device = true) left resident (colibri_print_model_resident); false also when `model` no longer holds
 *  what the device holds */
bool device_print_resident(const std::shared_ptr<void>& device, const TrainResult& model, const std::unordered_map<unsigned int, std::string>& classes, uint64_t tokens, bool loud,
                           std::ostream& out, bool instantiate = false);
/** which path printreverseindex() takes (environment COLIBRI_RINDEX = host | device | auto, with COLIBRI_PRINT's semantics) and the number of corpus
 *  positions from which auto goes to the device: environment COLIBRI_RINDEX_MIN; unset (~0), auto stays on the host path (no break-even has been measured,
 *  DESIGN.md §5g) */
ReportMode rindex_mode();
uint64_t   rindex_min_positions();
/** printreverseindex()'s text for a model's keys over a corpus payload, written to `out` (colibri_upload_corpus + colibri_print_classes + colibri_rindex +
 *  colibri_rindex_text). false = the host path has to do it (nothing was written), as device_print */
bool device_rindex_text(const std::unordered_map<unsigned int, std::string>& classes, const uint64_t* key_off, const unsigned char* key_bytes, uint64_t npatterns,
                        const unsigned char* payload, uint64_t nbytes, bool loud, std::ostream& out);
/** the same on the model and corpus a device_train(..., keep_device = true) left resident (colibri_rindex_resident) */
bool device_rindex_text_resident(const std::shared_ptr<void>& device, const TrainResult& model, const std::unordered_map<unsigned int, std::string>& classes, bool loud, std::ostream& out);
/** which path query() / querypatterns() take (environment COLIBRI_QUERY = host | device | auto, with COLIBRI_PRINT's semantics); auto stays on the host
 *  path: no break-even has been measured */
ReportMode query_mode();
/** the text of one batch of query lines (class-encoded, each closed by the delimiter byte; exact: one byte per line) for a model in export layout, written
 *  to `out` (colibri_print_classes + colibri_query + colibri_query_text). false = the host path has to do it (nothing was written), as device_print */
bool device_query(const std::unordered_map<unsigned int, std::string>& classes, const uint64_t* key_off, const unsigned char* key_bytes, const uint32_t* counts, uint64_t npatterns,
                  uint64_t tokens, const std::vector<unsigned char>& payload, const std::vector<unsigned char>& exact, uint32_t first_line, int minlength, int maxlength, bool loud,
                  std::ostream& out);
/** which path train()'s subsumption prunes (PRUNENONSUBSUMED / PRUNESUBSUMED) take (environment COLIBRI_SUBSUME = host | device | auto, with
 *  COLIBRI_PRINT's semantics) and the number of patterns from which auto goes to the device: environment COLIBRI_SUBSUME_MIN, else 10^6 (the smallest
 *  model on which the device route was measured ahead for the whole train() call beyond the boxes' spread) */
ReportMode subsume_mode();
uint64_t   subsume_min_patterns();
/** the flags and the per-length counts of the two prunes over a model's keys in export layout (colibri_subsume + colibri_subsume_fetch): keep gets one
 *  byte per pattern, pruned_non / pruned_sub COLIBRI_MAX_ORDER entries each, by the tokens of the pruned patterns. false = the host path has to do it
 *  (nothing was changed): no device layer or device — unless `loud`, which turns each of those into an error */
bool device_subsume(const uint64_t* key_off, const unsigned char* key_bytes, uint64_t npatterns, int prunenonsubsumed, int prunesubsumed, int maxlength, bool loud,
                    std::vector<uint8_t>& keep, uint64_t* pruned_non, uint64_t* pruned_sub);
/** the same on the model a device_train(..., keep_device = true) left resident (colibri_subsume_resident); false also when `model` no longer holds what
 *  the device holds */
bool device_subsume_resident(const std::shared_ptr<void>& device, const TrainResult& model, int prunenonsubsumed, int prunesubsumed, int maxlength, bool loud,
                             std::vector<uint8_t>& keep, uint64_t* pruned_non, uint64_t* pruned_sub);
/** which path trainskipgrams_selfconstrained() takes (environment COLIBRI_RECOUNT = host | device | auto): auto is the device, the in-place rebuild
 *  that leads to it already ran there and there is no earlier behaviour to keep */
ReportMode recount_mode();
/** the skipgrams `keys` counted on a corpus (colibri_recount + colibri_recount_fetch) into out's key, count and, for an indexed call, reference arrays,
 *  aligned to the keys: on the context `device` still holds the corpus on (a device_train(..., keep_device = true)), else on the payload, uploaded
 *  with `firstsentence`. Returns whether the resident corpus served. Errors are raised as device_train's are */
bool device_recount(const std::shared_ptr<void>& device, const unsigned char* payload, uint64_t nbytes, uint32_t firstsentence, const ConstraintKeys& keys, bool indexed,
                    uint32_t mintokens, TrainResult& out);
/** what a colibri_modelskip call looked at: `orders` orders from 3 on (the last may have found nothing: the loop ended there, before any prune), and by
 *  the order n the skipgrams found, the patterns of n tokens pruned below MINTOKENS (n-grams too) and the skipgrams pruned below MINSKIPTYPES */
struct SkipgramLog {
    uint32_t orders = 0;
    uint64_t found[COLIBRI_MAX_ORDER] = {0}, pruned[COLIBRI_MAX_ORDER] = {0}, extra[COLIBRI_MAX_ORDER] = {0};
};
/** the skipgrams of an indexed model of n-grams given in export layout (colibri_modelskip + colibri_modelskip_fetch + colibri_modelskip_info; DESIGN.md
 *  §5m); o: MINTOKENS (-1: 2), MINTOKENS_SKIPGRAMS, MINSKIPTYPES, MAXLENGTH and MAXSKIPS are read. Errors are raised as device_train's are */
void device_modelskip(const std::vector<uint64_t>& key_off, const unsigned char* key_bytes, const std::vector<uint64_t>& ref_off, const uint32_t* ref_sentence,
                      const uint16_t* ref_token, const colibri_options& o, SkipgramAnswer& out, SkipgramLog& log);
/** the same on the model a device_train(..., keep_device = true) left resident (colibri_modelskip_resident), which stays as it is; false (nothing done)
 *  when `model` no longer holds what the device holds or the run was not a single-device one */
bool device_modelskip_resident(const std::shared_ptr<void>& device, const TrainResult& model, const colibri_options& o, SkipgramAnswer& out, SkipgramLog& log);
/** distinct counts ascending and the patterns of each, for the patterns of one (category, size) group, 0 = all (colibri_histogram + colibri_histogram_fetch) */
struct HistogramRows {
    std::vector<uint32_t> counts;
    std::vector<uint64_t> patterns;
};
bool device_histogram(const uint64_t* key_off, const unsigned char* key_bytes, const uint32_t* counts, const uint64_t* ref_off, uint64_t npatterns, int category, uint64_t size,
                      bool loud, HistogramRows& out);
bool device_histogram_resident(const std::shared_ptr<void>& device, const TrainResult& model, int category, uint64_t size, bool loud, HistogramRows& out);
/** the per-order progress lines the reference prints while training (patternmodel.h:1005-1019, :1195-1245) */
void print_training_log(const colibri_stats& s, const colibri_options& o, std::ostream& err);
/** the tokens of a key as byte strings, gaps included (what the reference's pattern.ngrams(…, 1) yields, src/pattern.cpp:1284-1296) */
void token_slices(const unsigned char* data, size_t bytes, std::vector<std::string>& out);
/** the column legends the reference writes to stderr after print() (:2306-2320, :2918-2927) and report() (:2591-2600) */
void print_legend(std::ostream& err, bool indexed);
void report_legend(std::ostream& err, bool indexed);
/** reads one pattern of a model file in the given class-encoding version (1 or 2) and returns it v2-encoded */
Pattern read_model_pattern(std::istream& in, unsigned char classencodingversion);

inline void value_from_result(const TrainResult& r, size_t j, uint32_t& v) { v = r.counts[j]; }
inline void value_from_result(const TrainResult& r, size_t j, IndexedData& v) {
    v.data.clear();
    if (r.ref_off.empty()) return;
    for (uint64_t k = r.ref_off[j]; k < r.ref_off[j + 1]; ++k) v.data.push_back(IndexReference(r.ref_sentence[k], r.ref_token[k]));
}
inline void write_value_from_result(std::ostream& out, const TrainResult& r, size_t j, const uint32_t*) { out.write((const char*)&r.counts[j], sizeof(uint32_t)); }
inline void write_value_from_result(std::ostream& out, const TrainResult& r, size_t j, const IndexedData*) {
    const uint32_t c = r.ref_off.empty() ? 0 : (uint32_t)(r.ref_off[j + 1] - r.ref_off[j]);
    out.write((const char*)&c, sizeof(uint32_t));
    // the 6-byte (u32 sentence, u16 token) records of the file format (reference include/datatypes.h:60-63), packed in blocks: one stream write per block
    // instead of two per reference
    unsigned char  buf[6 * 1024];
    const uint64_t a = r.ref_off.empty() ? 0 : r.ref_off[j];
    for (uint32_t k = 0; k < c;) {
        const uint32_t n = std::min<uint32_t>(c - k, 1024u);
        for (uint32_t q = 0; q < n; ++q) {
            std::memcpy(buf + 6 * q, &r.ref_sentence[a + k + q], 4);
            std::memcpy(buf + 6 * q + 4, &r.ref_token[a + k + q], 2);
        }
        out.write((const char*)buf, (std::streamsize)(6 * n));
        k += n;
    }
}
/** Look-ups on a device result that is still flat arrays: an open-addressed table (slot -> pattern number + 1) over the keys, built by several host threads the first
 *  time a caller asks for a pattern. The reference's callers look patterns up right after train() (src/test.cpp:1214-1232, src/benchmarks.cpp:232-236); turning the
 *  9.4 M patterns of a 10^8-token model into unordered_map nodes first cost 2.6-3.1 s (one heap Pattern per node), this costs tens of milliseconds. The node map is
 *  still built when a caller iterates, inserts or asks for an iterator / a non-trivial value object. */
class FlatIndex {
  public:
    explicit FlatIndex(const TrainResult& r) : r_(r) { build(); }
    /** pattern number of the key, or (size_t)-1 */
    size_t find(const unsigned char* key, size_t n) const {
        if (r_.size() == 0) return (size_t)-1;
        for (uint64_t s = hash(key, n) & mask_;; s = (s + 1) & mask_) {
            const uint32_t e = table_.get()[s];
            if (e == 0) return (size_t)-1;
            const size_t j = e - 1;
            if ((size_t)(r_.key_off[j + 1] - r_.key_off[j]) == n && std::memcmp(r_.key_bytes.data() + r_.key_off[j], key, n) == 0) return j;
        }
    }

  private:
    static uint64_t hash(const unsigned char* p, size_t n) {  // (any well-mixed hash: the table is private to this process)
        uint64_t h = 0x9E3779B97F4A7C15ull ^ (uint64_t)n;
        while (n >= 8) {
            uint64_t w;
            std::memcpy(&w, p, 8);
            h = (h ^ w) * 0xff51afd7ed558ccdULL;
            h ^= h >> 32;
            p += 8;
            n -= 8;
        }
        uint64_t w = 0;
        std::memcpy(&w, p, n);
        h = (h ^ w) * 0xc4ceb9fe1a85ec53ULL;
        h ^= h >> 29;
        h *= 0xff51afd7ed558ccdULL;
        return h ^ (h >> 32);
    }
    void build() {
        const size_t n = r_.size();
        if (n == 0 || n >= 0xFFFFFFFFull) {
            if (n) throw InternalError();
            return;
        }
        uint64_t slots = 64;
        while (slots < n + n / 2) slots <<= 1;
        mask_ = slots - 1;
        table_.reset(static_cast<uint32_t*>(std::calloc(slots, sizeof(uint32_t))));  // (zero pages on first touch: the threads below fault them in)
        if (!table_) throw std::bad_alloc();
        unsigned nt = std::thread::hardware_concurrency();
        nt          = std::max(1u, std::min(nt ? nt : 4u, 32u));
        if (n < 200000) nt = 1;
        uint32_t* const tab = table_.get();
        auto            job = [this, tab, n, nt](unsigned t) {
            const size_t a = n * t / nt, b = n * (t + 1) / nt;
            for (size_t j = a; j < b; ++j) {
                const unsigned char* k = r_.key_bytes.data() + r_.key_off[j];
                const size_t         m = (size_t)(r_.key_off[j + 1] - r_.key_off[j]);
                for (uint64_t s = hash(k, m) & mask_;; s = (s + 1) & mask_) {
                    uint32_t expect = 0;
                    if (__atomic_compare_exchange_n(&tab[s], &expect, (uint32_t)(j + 1), false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) break;
                }
            }
        };
        if (nt == 1) {
            job(0);
        } else {
            std::vector<std::thread> th;
            for (unsigned t = 0; t < nt; ++t) th.emplace_back(job, t);
            for (auto& x : th) x.join();  // (join = the table's writes are visible to the caller)
        }
    }
    struct Free {
        void operator()(uint32_t* p) const { std::free(p); }
    };
    const TrainResult&              r_;
    std::unique_ptr<uint32_t, Free> table_;
    uint64_t                        mask_ = 0;
};

template <class V>
struct is_indexed_value {
    static const bool value = false;
};
template <>
struct is_indexed_value<IndexedData> {
    static const bool value = true;
};

}  // namespace colibri_host

/**
 * A pattern model: pattern -> value (count, or index of occurrences). reference include/patternmodel.h:546-2674.
 */
template <class ValueType, class ValueHandler = BaseValueHandler<ValueType>, class MapType = PatternMap<ValueType>>
class PatternModel : public MapType, public PatternModelInterface {
  protected:
    unsigned char model_type, model_version;
    uint64_t      totaltokens, totaltypes;
    int           maxn, minn;
    bool          hasskipgrams_;
    bool          types_settled_ = false;  // a threshold-1 run already asked for its word types (reference :1201-1207): its statistics cache is no longer
                                           // empty, so types() does not compute them again — a pattern list without one-token lines keeps 0 types
    ValueHandler  valuehandler;
    std::shared_ptr<colibri_host::TrainResult> result;  // device results not yet turned into map nodes
    mutable std::shared_ptr<colibri_host::FlatIndex> flatindex;  // ... and the look-up table over them (built by the first has() / occurrencecount())
    /** pattern number in the pending device result, (size_t)-1 if absent; only meaningful while `result` is set */
    size_t flat_find(const Pattern& p) const { return flat_find(p.data, p.bytesize()); }
    /** the same for key bytes that are not a Pattern of their own (a PatternPointer's): no copy into a heap Pattern per look-up. The table is built once, under a lock:
     * read-only look-ups on a fresh model from several threads are as safe as the reference's */
    size_t flat_find(const unsigned char* bytes, size_t n) const {
        std::shared_ptr<colibri_host::FlatIndex> f = std::atomic_load(&flatindex);
        if (!f) {
            std::lock_guard<std::mutex> l(flat_mutex());
            f = std::atomic_load(&flatindex);
            if (!f) {
                f = std::make_shared<colibri_host::FlatIndex>(*result);
                std::atomic_store(&flatindex, f);
            }
        }
        return f->find(bytes, n);
    }
    static std::mutex& flat_mutex() {
        static std::mutex m;
        return m;
    }
    static unsigned int flat_count(const colibri_host::TrainResult& r, size_t j) {
        return colibri_host::is_indexed_value<ValueType>::value ? (r.ref_off.empty() ? 0u : (unsigned int)(r.ref_off[j + 1] - r.ref_off[j])) : (unsigned int)r.counts[j];
    }

    void install_result(std::shared_ptr<colibri_host::TrainResult> r) {
        result = r;
        flatindex.reset();
        this->data.clear();
        PatternModel* self = this;
        this->pending_size = [r]() { return r->size(); };
        this->pending_fill = [self, r]() {
            self->data.reserve(r->size());
            for (size_t j = 0; j < r->size(); ++j) {
                ValueType v{};
                colibri_host::value_from_result(*r, j, v);
                self->data.emplace(Pattern(r->key_bytes.data() + r->key_off[j], (size_t)(r->key_off[j + 1] - r->key_off[j])), std::move(v));
            }
            self->flatindex.reset();
            self->result.reset();
        };
    }

  public:
    IndexedCorpus* reverseindex;
    bool           reverseindex_internal;

    /** empty model, optionally attached to a preloaded corpus (reference :644) */
    PatternModel<ValueType, ValueHandler, MapType>(IndexedCorpus* corpus = NULL)
        : model_type(0), model_version(2), totaltokens(0), totaltypes(0), maxn(0), minn(999), hasskipgrams_(false), reverseindex(corpus), reverseindex_internal(false) {
        model_type = (unsigned char)this->getmodeltype();
    }
    /** load from stream / file (reference :670, :700) */
    PatternModel<ValueType, ValueHandler, MapType>(std::istream* f, const PatternModelOptions& options, PatternModelInterface* constrainmodel = NULL, IndexedCorpus* corpus = NULL)
        : PatternModel(corpus) {
        this->load(*f, options, constrainmodel);
    }
    PatternModel<ValueType, ValueHandler, MapType>(const std::string& filename, const PatternModelOptions& options, PatternModelInterface* constrainmodel = NULL,
                                                   IndexedCorpus* corpus = NULL)
        : PatternModel(corpus) {
        if (!options.QUIET) std::cerr << "Loading " << filename << std::endl;
        std::ifstream in(filename, std::ios::in | std::ios::binary);
        if (!in.good()) {
            std::cerr << "ERROR: Unable to load file " << filename << std::endl;
            throw InternalError();
        }
        this->load(in, options, constrainmodel);
    }
    virtual ~PatternModel() {
        if (reverseindex_internal) delete reverseindex;
    }

    int getmodeltype() const override { return colibri_host::is_indexed_value<ValueType>::value ? INDEXEDPATTERNMODEL : UNINDEXEDPATTERNMODEL; }
    int getmodelversion() const override { return 2; }
    PatternModelInterface* getinterface() { return (PatternModelInterface*)this; }

    size_t       size() const override { return MapType::size(); }
    bool         has(const Pattern& p) const override { return result ? flat_find(p) != (size_t)-1 : MapType::has(p); }
    bool         has(const PatternPointer& p) const override {
        if (result && p.mask == 0) return flat_find(p.data, (size_t)p.bytes) != (size_t)-1;  // (an unmasked pointer's bytes ARE the key: no heap Pattern per look-up)
        return this->has(Pattern(p));
    }
    int          maxlength() const override { return maxn; }
    int          minlength() const override { return minn; }
    unsigned int types() override {  // a loaded model without a type count falls back to the word types its patterns hold (reference :1700-1704)
        if (totaltypes == 0 && this->size() != 0 && !types_settled_) totaltypes = this->totalwordtypesingroup(0, 0);
        return (unsigned int)totaltypes;
    }
    unsigned int tokens() const override { return (unsigned int)totaltokens; }
    unsigned char type() const { return model_type; }
    unsigned char version() const { return model_version; }
    bool          hasskipgrams() const { return hasskipgrams_; }

  protected:
    // the gap masks of the model's skipgrams by length, ascending (what the reference's matchskipgramhelper walks, without its index by first word)
    std::map<int, std::vector<uint32_t>> skipmasks_;
    size_t                                skipmasks_size_ = (size_t)-1;
    void compute_skipmasks() {
        if (skipmasks_size_ == this->size()) return;
        skipmasks_.clear();
        std::set<std::pair<int, uint32_t>> seen;
        for (typename MapType::iterator it = this->begin(); it != this->end(); ++it) {
            if (it->first.category() != SKIPGRAM) continue;
            std::vector<std::string> toks;
            colibri_host::token_slices(it->first.data, it->first.bytesize(), toks);
            uint32_t mask = 0;
            for (size_t k = 0; k < toks.size() && k < 31; ++k)
                if (toks[k].size() == 1 && (unsigned char)toks[k][0] == colibri_classes::skipclass) mask |= (1u << k);
            if (seen.insert(std::make_pair((int)toks.size(), mask)).second) skipmasks_[(int)toks.size()].push_back(mask);
        }
        for (std::map<int, std::vector<uint32_t>>::iterator it = skipmasks_.begin(); it != skipmasks_.end(); ++it) std::sort(it->second.begin(), it->second.end());
        skipmasks_size_ = this->size();
    }
    bool     instances_checked_     = false;  // print(out, decoder, true) has checked every row's instances: the rows it prints do not check again
    uint32_t trained_firstsentence_ = 1;  // the sentence number the last train() gave the corpus' first sentence

  public:
    /**
     * The patterns of the model that start at `ref` of the loaded corpus (reference :1746-1824), in the defined order: n ascending from minlength() to
     * maxlength() while the window fits its sentence, the n-gram before its skipgrams, gap masks ascending. The n-gram window counts when the model has it;
     * for n >= 3 the window under every gap mask a skipgram of the model has at that length counts when the model has that key, also where the n-gram is
     * not in the model. occurrencecount > 0: the pattern's count must reach it; category 0 = any (NGRAM: no skipgrams; SKIPGRAM: no n-grams; FLEXGRAM:
     * nothing); size 0 = any length. This is the specification of the device's reverse index (csrc/rindex.hpp).
     */
    void reverseindex_ordered(const IndexReference& ref, unsigned int occurrencecount, int category, unsigned int size, std::vector<PatternPointer>& out) {
        if (reverseindex == NULL) return;
        const unsigned int sl    = reverseindex->sentencelength((int)ref.sentence);
        const bool         masks = category != NGRAM && category != FLEXGRAM && this->hasskipgrams();
        if (masks) compute_skipmasks();
        for (unsigned int n = (unsigned int)std::max(1, this->minlength()); ref.token + n <= sl && (int)n <= this->maxlength(); ++n) {
            if (size != 0 && n != size) continue;
            PatternPointer window = reverseindex->getpattern(ref, (int)n);
            if ((category == 0 || category == NGRAM) && this->has(window) && (occurrencecount == 0 || this->occurrencecount(Pattern(window)) >= occurrencecount)) out.push_back(window);
            if (!masks || n < 3) continue;
            std::map<int, std::vector<uint32_t>>::const_iterator it = skipmasks_.find((int)n);
            if (it == skipmasks_.end()) continue;
            for (uint32_t mask : it->second) {
                window.mask = mask;
                const Pattern skipgram(window);
                if (this->has(skipgram) && (occurrencecount == 0 || this->occurrencecount(skipgram) >= occurrencecount)) out.push_back(window);
            }
        }
    }
    /** the same as a set, as the reference returns it (:1746) */
    std::unordered_set<PatternPointer> getreverseindex(const IndexReference& ref, int occurrencecount = 0, int category = 0, unsigned int size = 0) {
        std::vector<PatternPointer> v;
        reverseindex_ordered(ref, (unsigned int)std::max(0, occurrencecount), category, size, v);
        return std::unordered_set<PatternPointer>(v.begin(), v.end());
    }
    /** every (position, pattern) of a sentence (1-based), positions ascending and each position's patterns in the defined order (reference :1849-1862) */
    std::vector<std::pair<IndexReference, PatternPointer>> getreverseindex_bysentence(int sentence, int occurrencecount = 0, int category = 0, unsigned int size = 0) {
        std::vector<std::pair<IndexReference, PatternPointer>> out;
        if (reverseindex == NULL) return out;
        const unsigned int          sl = reverseindex->sentencelength(sentence);
        std::vector<PatternPointer> v;
        for (unsigned int t = 0; t < sl; ++t) {
            const IndexReference ref((uint32_t)sentence, (uint16_t)t);
            v.clear();
            reverseindex_ordered(ref, (unsigned int)std::max(0, occurrencecount), category, size, v);
            for (const PatternPointer& pp : v) out.push_back(std::make_pair(ref, pp));
        }
        return out;
    }
    /**
     * The reverse index as text (reference :2325-2338): per real token position "s:t", then "\t<pattern text>" per pattern in the defined order, then
     * "\n"; one more "\n" after the last line. Sentences are 1-based and empty ones are counted. Nothing without a reverse index. COLIBRI_RINDEX = host |
     * device | auto: the host loop below is the specification; the device writes the same bytes from one call over the model (csrc/rindex.hpp), on the
     * model still resident after train() or on the uploaded one; auto stays on the host unless COLIBRI_RINDEX_MIN (positions) is set and reached.
     */
    virtual void printreverseindex(std::ostream& out, ClassDecoder& decoder) {
        if (reverseindex == NULL || reverseindex->empty()) return;
        if (printreverseindex_from_device(out, decoder)) return;
        std::vector<PatternPointer> v;
        const unsigned int          ns = reverseindex->sentences();
        for (unsigned int s = 1; s <= ns; ++s) {
            const unsigned int sl = reverseindex->sentencelength((int)s);
            for (unsigned int t = 0; t < sl; ++t) {
                const IndexReference ref(s, (uint16_t)t);
                v.clear();
                reverseindex_ordered(ref, 0, 0, 0, v);
                out << s << ':' << t;
                for (const PatternPointer& pp : v) out << "\t" << Pattern(pp).tostring(decoder);
                out << "\n";
            }
        }
        out << std::endl;
    }
    bool printreverseindex_from_device(std::ostream& out, const ClassDecoder& decoder) {
        const colibri_host::ReportMode mode = colibri_host::rindex_mode();
        if (mode == colibri_host::REPORT_HOST) return false;
        const bool loud = mode == colibri_host::REPORT_DEVICE;
        if (!loud) {
            uint64_t positions = 0;
            const uint64_t min = colibri_host::rindex_min_positions();
            if (min == ~0ull) return false;
            for (unsigned int s = 1; s <= reverseindex->sentences() && positions < min; ++s) positions += reverseindex->sentencelength((int)s);
            if (positions < min) return false;
        }
        bool done = false, resident = false;
        if (result && result->device && trained_firstsentence_ == 1) done = resident = colibri_host::device_rindex_text_resident(result->device, *result, decoder.words(), loud, out);
        if (!done) {
            FlatView v;
            if (!flat_view(v, false, 0)) {
                if (loud) std::cerr << "ERROR: COLIBRI_RINDEX=device, but this model has no device form (an indexed model over unindexed results): the host path prints" << std::endl;
                return false;
            }
            done = colibri_host::device_rindex_text(decoder.words(), v.ko, v.kb, v.np, reverseindex->beginpointer(), reverseindex->bytesize(), loud, out);
        }
        if (!done) return false;
        out.flush();
        if (loud) std::cerr << "(reverse index on the device: " << (resident ? "resident" : "uploaded") << " model)" << std::endl;
        return true;
    }
    /**
     * The patterns of the model that occur in `pattern`, with the token they start at (reference :2272-2285): the windows of minlength() .. maxlength()
     * tokens, size by size, left to right, that the model has. No skipgram is matched against a gap-free pattern (the reference's TODO). A model fresh
     * from the device answers from its flat arrays (has()).
     */
    std::vector<std::pair<Pattern, int>> getpatterns(const Pattern& pattern) {
        std::vector<std::pair<Pattern, int>> v, ngrams;
        pattern.subngrams(ngrams, this->minlength(), this->maxlength());
        for (const auto& w : ngrams)
            if (this->has(w.first)) v.push_back(w);
        return v;
    }
    /**
     * A batch of query lines (the reference's -Q loop, src/patternmodeller.cpp:187-231, over a whole stream): line L counts every line from first_line;
     * "X" switches between extensive mode (the default: "L:0" and the row of the whole line when the model has it, then "L:i" and the row of every
     * pattern getpatterns() finds) and exact mode (the row of the line, or PATTERN "..." NOT FOUND IN MODEL); empty lines print nothing. A row is the
     * plain model's (text, count, coverage count, coverage, category, size, frequency), also for an indexed model: that is what the reference's query
     * prints. COLIBRI_QUERY = host | device | auto: the host loop is the specification; the device answers the whole batch from one call over the
     * model (csrc/query.hpp), uploaded through flat_view with its counts; auto stays on the host.
     */
    void query(std::istream& lines, ClassEncoder& encoder, const ClassDecoder& decoder, std::ostream& out, uint32_t first_line = 1) {
        std::vector<QueryLine> batch;
        std::string            line;
        bool                   exact = false;
        while (std::getline(lines, line)) {
            QueryLine q;
            if (line == "X") {
                exact = !exact;
            } else if (!line.empty()) {
                q.active = true;
                q.exact  = exact;
                encode_queryline(encoder, line, q.key);
            }
            batch.push_back(q);
        }
        run_query(batch, decoder, out, first_line);
    }
    /** the rows of -q (reference src/patternmodeller.cpp:171-185): every string as a line of exact mode */
    void querypatterns(const std::vector<std::string>& patterns, ClassEncoder& encoder, const ClassDecoder& decoder, std::ostream& out) {
        std::vector<QueryLine> batch(patterns.size());
        for (size_t j = 0; j < patterns.size(); ++j) {
            batch[j].active = batch[j].exact = true;
            encode_queryline(encoder, patterns[j], batch[j].key);
        }
        run_query(batch, decoder, out, 1);
    }

  protected:
    struct QueryLine {
        std::vector<unsigned char> key;  // the line's key bytes
        bool                       active = false, exact = false;  // active: neither empty nor the mode switch
    };
    static void encode_queryline(ClassEncoder& encoder, const std::string& line, std::vector<unsigned char>& key) {
        const Pattern p = encoder.buildpattern(line, true);
        key.assign(p.data, p.data + p.bytesize());
    }
    /** the row the reference's query prints for a pattern of the model: print()'s without what an indexed model adds */
    void print_queryrow(std::ostream& out, const ClassDecoder& decoder, const Pattern& pattern) {
        const unsigned int count    = this->occurrencecount(pattern);
        const size_t       covcount = this->coveragecount(pattern);
        const int          cat      = (int)pattern.category();
        out << pattern.tostring(decoder) << "\t" << count << "\t" << covcount << "\t" << covcount / (double)this->tokens() << "\t"
            << (cat == NGRAM ? "ngram" : cat == SKIPGRAM ? "skipgram" : cat == FLEXGRAM ? "flexgram" : "") << "\t" << pattern.size() << "\t" << this->frequency(pattern) << std::endl;
    }
    void run_query(const std::vector<QueryLine>& batch, const ClassDecoder& decoder, std::ostream& out, uint32_t first_line) {
        if (query_from_device(batch, decoder, out, first_line)) return;
        for (size_t j = 0; j < batch.size(); ++j) {
            const QueryLine& q = batch[j];
            if (!q.active) continue;
            const Pattern  p(q.key.data(), q.key.size());
            const bool     found = !q.key.empty() && this->has(p);
            const uint32_t L     = first_line + (uint32_t)j;
            if (q.exact) {
                if (found) print_queryrow(out, decoder, p);
                else out << "PATTERN \"" << p.tostring(decoder) << "\" NOT FOUND IN MODEL" << std::endl;
                continue;
            }
            if (q.key.empty()) continue;
            const std::vector<std::pair<Pattern, int>> patterns = this->getpatterns(p);
            if (found) {
                out << L << ':' << 0 << "\t";
                print_queryrow(out, decoder, p);
            }
            for (const auto& w : patterns) {
                out << L << ':' << (int)(uint16_t)w.second << "\t";
                print_queryrow(out, decoder, w.first);
            }
        }
    }
    bool query_from_device(const std::vector<QueryLine>& batch, const ClassDecoder& decoder, std::ostream& out, uint32_t first_line) {
        const colibri_host::ReportMode mode = colibri_host::query_mode();
        if (mode != colibri_host::REPORT_DEVICE) return false;  // (auto: no break-even has been measured, the host loop answers)
        const bool indexed = colibri_host::is_indexed_value<ValueType>::value;
        if (!colibri_host::stream_in_default_float_state(out)) {
            std::cerr << "ERROR: COLIBRI_QUERY=device, but the stream is not in its default float state: the host path prints" << std::endl;
            return false;
        }
        std::vector<unsigned char> payload, exact;
        for (const QueryLine& q : batch) {
            payload.insert(payload.end(), q.key.begin(), q.key.end());
            payload.push_back(0);
            exact.push_back(q.active && q.exact ? 1 : 0);
        }
        // The model goes up with its counts, whether it is fresh from the device or not: the only models train() leaves resident are indexed ones
        // (with skipgrams), whose resident rows would carry their references, which the reference's query rows do not.
        FlatView v;
        if (!flat_view(v, false, 0)) {
            std::cerr << "ERROR: COLIBRI_QUERY=device, but this model has no device form (an indexed model over unindexed results): the host path prints" << std::endl;
            return false;
        }
        std::vector<uint32_t> counts;
        if (indexed) {
            counts.resize(v.np + 1);
            for (uint64_t j = 0; j < v.np; ++j) counts[j] = (uint32_t)(v.ro[j + 1] - v.ro[j]);
        }
        const bool done = colibri_host::device_query(decoder.words(), v.ko, v.kb, indexed ? counts.data() : v.ct, v.np, this->tokens(), payload, exact, first_line, this->minlength(),
                                                     this->maxlength(), true, out);
        if (!done) return false;
        out.flush();
        std::cerr << "(query on the device: uploaded model)" << std::endl;
        return true;
    }

  public:
    /** does nothing for unindexed models (reference :2653-2655); IndexedPatternModel abstracts its skipgrams on the device */
    virtual int computeflexgrams_fromskipgrams() { return 0; }
    /** does nothing for unindexed models (reference :2628) */
    virtual void outputrelations(const Pattern&, const ClassDecoder&, std::ostream&, const std::string& = "", bool = true) {}
    /** the CLI's relation loop (reference src/patternmodeller.cpp:274-285): every pattern, then its relations; unindexed models have none */
    virtual void outputrelations_model(const ClassDecoder& classdecoder, std::ostream& OUT, const std::string&) {
        for (typename MapType::iterator it = this->begin(); it != this->end(); ++it) OUT << it->first.tostring(classdecoder) << std::endl;
    }
    /** do nothing for unindexed models, not even a header (reference :2659-2660) */
    virtual void outputcooc_npmi(std::ostream&, const ClassDecoder&, double) {}
    virtual void outputcooc(std::ostream&, const ClassDecoder&, double) {}
    /** what the reference's constrained in-place rebuild leaves in the type count: the number of patterns the model was loaded with
     *  (it takes "total word types prior to pruning" from a map that already holds every pattern, patternmodel.h:1197-1201) */
    void settypes_inplace_rebuild() { totaltypes = this->size(); }

    bool collect_keys(std::vector<uint64_t>& off, std::vector<unsigned char>& bytes) override {
        off.assign(1, 0);
        bytes.clear();
        if (result) {  // device results not materialised yet: their flat arrays are exactly what is wanted
            off   = result->key_off;
            bytes = result->key_bytes;
            return true;
        }
        for (typename MapType::iterator it = this->begin(); it != this->end(); ++it) {
            const size_t n = it->first.bytesize();
            bytes.insert(bytes.end(), it->first.data, it->first.data + n);
            off.push_back(bytes.size());
        }
        return true;
    }
    /** keys and counts in export layout, in the model's iteration order (a device result not yet materialised: its flat arrays) */
    void collect_counts(std::vector<uint64_t>& off, std::vector<unsigned char>& bytes, std::vector<uint32_t>& counts) {
        collect_keys(off, bytes);
        counts.clear();
        if (result) {
            counts.reserve(result->size());
            for (size_t j = 0; j < result->size(); ++j) counts.push_back(flat_count(*result, j));
            return;
        }
        counts.reserve(this->size());
        for (typename MapType::iterator it = this->begin(); it != this->end(); ++it) counts.push_back(valuehandler.count(it->second));
    }
    ValueType* getdata(const Pattern& pattern, bool makeifnew = false) {
        typename MapType::iterator it = this->find(pattern);
        if (it != this->end()) return &(it->second);
        if (makeifnew) return &((*this)[pattern]);
        return NULL;
    }
    unsigned int occurrencecount(const Pattern& pattern) override {
        if (result) {  // a model fresh from the device: answered from its flat arrays
            const size_t j = flat_find(pattern);
            return j == (size_t)-1 ? 0u : flat_count(*result, j);
        }
        ValueType* v = getdata(pattern, false);
        return v ? valuehandler.count(*v) : 0;
    }
    /** the pattern's share of the occurrences of its own (category, size) group (reference :2047-2050) */
    double frequency(const Pattern& pattern) override { return this->occurrencecount(pattern) / (double)totaloccurrencesingroup((int)pattern.category(), (int)pattern.n()); }
    /** host-side add of one occurrence (reference :2059-2073); training itself never calls this, it is here for callers that extend a model */
    virtual void add(const Pattern& pattern, const IndexReference& ref) { valuehandler.add(getdata(pattern, true), ref); }
    /** erase patterns under a threshold, optionally only of size _n (reference :2107-2128) */
    unsigned int prune(int threshold, int _n = 0) {
        unsigned int pruned = 0;
        for (typename MapType::iterator it = this->begin(); it != this->end();) {
            if ((_n == 0 || (int)it->first.n() == _n) && (threshold == -1 || valuehandler.count(it->second) < (unsigned int)threshold)) {
                it = this->data.erase(it);
                ++pruned;
            } else {
                ++it;
            }
        }
        return pruned;
    }

    /**
     * Train on class-encoded corpus data — same signature as reference include/patternmodel.h:880-881.
     * `in` may be NULL when a preloaded corpus (reverse index) is attached.
     */
    virtual void train(std::istream* in, const PatternModelOptions& in_options, PatternModelInterface* constrainbymodel = NULL, PatternSet<>* filter = NULL, bool continued = false,
                       uint32_t firstsentence = 1, bool ignoreerrors = false) {
        (void)ignoreerrors;
        PatternModelOptions options = in_options;
        if (options.MINTOKENS == -1) options.MINTOKENS = 2;
        if (options.MINTOKENS == 0) options.MINTOKENS = 1;
        if (options.MINTOKENS_SKIPGRAMS < options.MINTOKENS) options.MINTOKENS_SKIPGRAMS = options.MINTOKENS;
        if (filter != NULL && filter->size() == 0) filter = NULL;  // cython passes empty sets (reference :902-903)
        if (filter != NULL && constrainbymodel != NULL) filter = NULL;  // the reference only consults the filter in unconstrained runs (:1106)
        if (continued && (constrainbymodel != NULL || (this->data.empty() && !result))) continued = false;  // nothing to continue from / a constrained run counts everything anyway (:985)
        if (continued) {
            train_continued(in, options, firstsentence);
            return;
        }
        // Constrained training (reference :1062-1072, :1088-1089): one pass over all lengths, a window counts iff the constraint model has it.
        // The keys of the constraint model become a device-side set (colibri_set_constraint). constrainbymodel == this is the in-place
        // rebuild of patternmodeller -I / -2: the model's own patterns are the constraint, then it is emptied and rebuilt.
        const bool                   inplace = constrainbymodel == (PatternModelInterface*)this;
        colibri_host::ConstraintKeys ck, skipkeys;
        const bool                   recount = inplace && options.DOSKIPGRAMS && !options.DOSKIPGRAMS_EXHAUSTIVE;  // -I -s
        uint64_t                     constraint_tokens = 0, constraint_types = 0, loaded_patterns = 0;
        if (constrainbymodel != NULL) {
            if (options.DOSKIPGRAMS && !options.DOSKIPGRAMS_EXHAUSTIVE && !inplace) {  // reference :941-956
                options.DOSKIPGRAMS            = false;
                options.DOSKIPGRAMS_EXHAUSTIVE = true;
                if (!options.QUIET)
                    std::cerr << "WARNING: Skipgrams will be extracted exhaustively on the basis of the ngrams found; the constraint model will be applied only afterwards. "
                                 "This implies some skipgrams in the constraint model that are present may be missed, and it will not be most efficient. Use in-place "
                                 "rebuilding of your constraint model instead."
                              << std::endl;
            }
            if (inplace && options.DOSKIPGRAMS_EXHAUSTIVE) {
                std::cerr << "ERROR: exhaustive skipgrams in an in-place constrained rebuild are not on the MI355X-accelerated path" << std::endl;
                throw InternalError();
            }
            if (!constrainbymodel->collect_keys(ck.off, ck.bytes)) {
                std::cerr << "ERROR: the constraint model cannot enumerate its patterns; pass a PatternModel / PatternSetModel of this build" << std::endl;
                throw InternalError();
            }
            if (inplace && options.DOSKIPGRAMS) {
                // the model's own skipgrams are set aside: the one pass below counts n-grams only (reference :1212-1215), trainskipgrams_selfconstrained
                // counts them afterwards (:1271-1273)
                colibri_host::ConstraintKeys ngrams;
                ngrams.off.assign(1, 0);
                skipkeys.off.assign(1, 0);
                for (size_t k = 0; k + 1 < ck.off.size(); ++k) {
                    const unsigned char*  key = ck.bytes.data() + ck.off[k];
                    const size_t          nb  = (size_t)(ck.off[k + 1] - ck.off[k]);
                    const PatternCategory cat = colibri_host::category_of(key, nb);
                    if (cat == FLEXGRAM) {
                        std::cerr << "ERROR: the loaded model holds flexgrams: an in-place rebuild with skipgrams (-I -s) would have to match them, which is not on the "
                                     "MI355X-accelerated path" << std::endl;
                        throw InternalError();
                    }
                    colibri_host::ConstraintKeys& to = cat == SKIPGRAM ? skipkeys : ngrams;
                    to.bytes.insert(to.bytes.end(), key, key + nb);
                    to.off.push_back(to.bytes.size());
                }
                ck.off.swap(ngrams.off);
                ck.bytes.swap(ngrams.bytes);
            }
            if (inplace) {
                loaded_patterns = this->size();
                this->data.clear();
                result.reset();
                flatindex.reset();
                this->pending_fill = nullptr;
                this->pending_size = nullptr;
                maxn = 0;
                minn = 999;
            } else {
                constraint_tokens = constrainbymodel->tokens();  // the reference starts its totals from the constraint model's (:892-895)
                constraint_types  = constrainbymodel->types();
            }
        }
        if (!this->data.empty() || result) {
            if (constrainbymodel != NULL || filter != NULL) {
                std::cerr << "ERROR: train() on a non-empty model with a constraint model or a filter is not on the MI355X-accelerated path" << std::endl;
                throw InternalError();
            }
            train_expand(in, options, firstsentence);  // the loaded model grows by this corpus (reference :880-1270 with continued = false; colibri-patternmodeller -e without -E)
            return;
        }
        colibri_host::ConstraintKeys fk;  // train(..., filter): the filter's patterns (reference :899-914, :1106-1133)
        if (filter != NULL) {
            if (options.DOSKIPGRAMS || options.DOSKIPGRAMS_EXHAUSTIVE || options.MINLENGTH > 1 || options.DOPATTERNPERLINE || options.MAXBACKOFFLENGTH < options.MAXLENGTH ||
                options.MINTOKENS_UNIGRAMS > options.MINTOKENS) {
                std::cerr << "ERROR: training with a filter is on the MI355X-accelerated path for MINLENGTH = 1, without skipgrams, back-off length, word threshold or pattern list"
                          << std::endl;
                throw InternalError();
            }
            bool hasngrams = false, hasother = false;
            fk.off.push_back(0);
            for (typename PatternSet<>::iterator it = filter->begin(); it != filter->end(); ++it) {
                (it->category() == NGRAM ? hasngrams : hasother) = true;
                fk.bytes.insert(fk.bytes.end(), it->data, it->data + it->bytesize());
                fk.off.push_back(fk.bytes.size());
            }
            if (!options.QUIET && hasngrams)
                std::cerr << "Filter with ngrams provided, only patterns that either match a filtered pattern or contain a smaller filtered pattern will be included..." << std::endl;
            if (!options.QUIET && hasother) std::cerr << "Filter with skipgrams provided, only matching instances will be included..." << std::endl;
        }
        if (!options.QUIET) std::cerr << "Training patternmodel, occurrence threshold: " << options.MINTOKENS << std::endl;

        colibri_options o{};
        o.mintokens              = options.MINTOKENS;
        o.maxlength              = options.MAXLENGTH;
        o.minlength              = (constrainbymodel == NULL) ? 1 : options.MINLENGTH;  // unconstrained: shorter patterns are dropped after the run (drop_short_patterns)
        o.maxbackofflength       = options.MAXBACKOFFLENGTH;
        o.mintokens_unigrams     = options.MINTOKENS_UNIGRAMS;
        o.mintokens_skipgrams    = options.MINTOKENS_SKIPGRAMS;
        o.minskiptypes           = options.MINSKIPTYPES;
        o.maxskips               = options.MAXSKIPS;
        o.doskipgrams            = options.DOSKIPGRAMS && !recount;
        o.doskipgrams_exhaustive = options.DOSKIPGRAMS_EXHAUSTIVE;
        o.dopatternperline       = options.DOPATTERNPERLINE;
        o.prunenonsubsumed       = 0;  // both subsumption prunes are post-hoc passes over the finished model (reference :1280-1330): done below, on the host
        o.prunesubsumed          = 0;
        o.indexed                = colibri_host::is_indexed_value<ValueType>::value ? 1 : 0;

        std::shared_ptr<colibri_host::TrainResult> r = std::make_shared<colibri_host::TrainResult>();
        // an indexed skipgram model stays resident on the device until it is materialised on the host: computeflexgrams_fromskipgrams works on it there
        const int  world = (constrainbymodel == NULL && filter == NULL && !options.DOPATTERNPERLINE) ? colibri_host::gpus() : 1;  // sentence-sharded over that many GPUs (src/sharded.cpp)
        const bool keep_device = (world == 1 && o.indexed && o.doskipgrams && constrainbymodel == NULL && options.MINLENGTH <= 1) ||
                                 (recount && skipkeys.off.size() > 1 && colibri_host::recount_mode() != colibri_host::REPORT_HOST);  // (the corpus stays uploaded for the skipgrams)
        if (world > 1 || (world == 1 && constrainbymodel == NULL && filter == NULL && !options.DOPATTERNPERLINE && std::getenv("COLIBRI_GPUS_FORCE_SHARDED") != NULL)) {  // (forced: the sharded protocol on one rank, for tests; a filtered run has no sharded form)
            std::vector<unsigned char> owned;
            const unsigned char*       p = NULL;
            uint64_t                   nb = 0;
            if (reverseindex != NULL && !reverseindex->empty()) {
                p  = reverseindex->beginpointer();
                nb = reverseindex->bytesize();
            } else if (in != NULL) {
                owned = colibri_host::read_corpus_payload(*in);
                p     = owned.data();
                nb    = owned.size();
            }
            if (p == NULL || nb == 0) {
                std::cerr << "ERROR: No corpus data to train on" << std::endl;
                throw InternalError();
            }
            colibri_host::device_train_sharded(p, nb, o, firstsentence, *r, world);
        } else if (reverseindex != NULL && !reverseindex->empty()) {
            colibri_host::device_train(reverseindex->beginpointer(), reverseindex->bytesize(), o, firstsentence, *r, constrainbymodel ? &ck : (filter ? &fk : NULL), keep_device,
                                       false, filter != NULL);
        } else if (in != NULL) {
            const std::vector<unsigned char> payload = colibri_host::read_corpus_payload(*in);
            if (payload.empty()) {
                std::cerr << "ERROR: Attempting to read pattern from file, but file is empty?" << std::endl;  // reference src/pattern.cpp:520-523
                throw InternalError();
            }
            colibri_host::device_train(payload.data(), payload.size(), o, firstsentence, *r, constrainbymodel ? &ck : (filter ? &fk : NULL), keep_device, false, filter != NULL);
        } else {
            std::cerr << "ERROR: No input stream and no reverse index (preloaded corpus) to train on" << std::endl;
            throw InternalError();
        }
        if (constrainbymodel == NULL && options.MINLENGTH > 1) colibri_host::drop_short_patterns(*r, options.MINLENGTH);
        trained_firstsentence_ = firstsentence;
        if (!options.QUIET) colibri_host::print_training_log(r->stats, o, std::cerr);
        totaltokens   = r->stats.totaltokens;
        totaltypes    = r->stats.totaltypes;
        if (constrainbymodel != NULL) {
            if (inplace) {
                // "total word types prior to pruning" is taken from a map that still holds every loaded pattern (:1197-1205): their number when
                // MINTOKENS > 1, the word types among the loaded unigrams when MINTOKENS == 1 (and MINLENGTH == 1), else left to types()
                if (options.MINTOKENS > 1) {
                    totaltypes = loaded_patterns;
                } else if (options.MINLENGTH == 1) {
                    uint64_t unigrams = 0;
                    for (size_t k = 0; k + 1 < ck.off.size(); ++k)
                        unigrams += colibri_host::token_count(ck.bytes.data() + ck.off[k], (size_t)(ck.off[k + 1] - ck.off[k])) == 1;
                    totaltypes = unigrams;
                } else {
                    totaltypes = 0;
                }
            } else {
                totaltokens += constraint_tokens;  // the corpus' tokens are added to the constraint model's total (:894, :1047-1048)
                totaltypes = constraint_types;
            }
        }
        if (r->stats.maxn > maxn) maxn = r->stats.maxn;
        if (r->stats.npatterns && r->stats.minn < minn) minn = r->stats.minn;
        hasskipgrams_ = (options.DOSKIPGRAMS || options.DOSKIPGRAMS_EXHAUSTIVE);
        types_settled_ = options.DOPATTERNPERLINE || (filter != NULL && options.MINTOKENS == 1);  // (a filter without one-token matches at threshold 1: 0 types, as above)
        const bool subsume = options.PRUNENONSUBSUMED || options.PRUNESUBSUMED;
        const auto t0      = std::chrono::steady_clock::now();
        const bool pruned  = subsume && !recount && prune_by_subsumption_on_device(*r, options);  // (the flat arrays, before they are installed: no node map is built; not ahead of -I -s's skipgrams)
        install_result(r);
        if (recount) {
            hasskipgrams_ = skipkeys.off.size() > 1;  // (what the load left)
            for (size_t k = 0; k + 1 < skipkeys.off.size(); ++k)
                (*this)[Pattern(skipkeys.bytes.data() + skipkeys.off[k], (size_t)(skipkeys.off[k + 1] - skipkeys.off[k]))] = ValueType{};
            recount_skipgrams(options, firstsentence, r->device);
            r->device.reset();
        }
        if (subsume && !pruned) prune_by_subsumption(options);
        if (subsume && std::getenv("COLIBRI_HOST_TIMING") != NULL)  // (with device_train's line: where the call's wall time goes)
            std::cerr << "COLIBRI_HOST_TIMING subsume " << std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() << " ms on the "
                      << (pruned ? "device" : "host") << ", " << this->size() << " patterns left" << std::endl;
    }

    /**
     * The skipgrams of the model counted anew on the attached corpus (reference :1569-1604; colibri-patternmodeller -I -s reaches it from train()
     * after the n-gram rebuild). A skipgram of n >= 3 tokens occurs at (s, t) when its window fits the sentence and every token outside its gaps
     * equals its own; MINSKIPTYPES, MINTOKENS_SKIPGRAMS and MAXSKIPS play no part. Every skipgram's value is replaced by what the corpus gives,
     * references ascending; then prune(MINTOKENS) runs over the whole model, as in the reference. firstsentence: the number of the corpus' first
     * sentence (0 = the last train()'s). COLIBRI_RECOUNT = host | device | auto: host is the loop over reverseindex_ordered() and needs no GPU;
     * device is colibri_recount (csrc/recount.hpp), on the context a train() just used where there is one; auto is device.
     */
    virtual void trainskipgrams_selfconstrained(const PatternModelOptions& options, uint32_t firstsentence = 0) {
        const uint32_t first = firstsentence ? firstsentence : trained_firstsentence_;
        // (a corpus a train() left on the device was uploaded with that run's sentence numbers)
        recount_skipgrams(options, first, result && first == trained_firstsentence_ ? result->device : std::shared_ptr<void>());
    }

  protected:
    void recount_skipgrams(const PatternModelOptions& in_options, uint32_t firstsentence, const std::shared_ptr<void>& device) {
        PatternModelOptions options = in_options;
        if (options.MINTOKENS == -1) options.MINTOKENS = 2;
        if (options.MINTOKENS == 0) options.MINTOKENS = 1;
        this->materialise();
        if (!options.QUIET) std::cerr << "Finding skipgrams/flexgrams matching preloaded constraints, occurrence threshold " << options.MINTOKENS << " ..." << std::endl;
        colibri_host::ConstraintKeys keys;
        std::vector<ValueType*>      values;
        keys.off.assign(1, 0);
        for (typename MapType::iterator it = this->begin(); it != this->end(); ++it) {
            const PatternCategory cat = it->first.category();
            if (cat == FLEXGRAM) {
                std::cerr << "ERROR: the model holds flexgrams: trainskipgrams_selfconstrained would have to match them, which is not on the MI355X-accelerated path" << std::endl;
                throw InternalError();
            }
            if (cat != SKIPGRAM) continue;
            it->second = ValueType{};
            keys.bytes.insert(keys.bytes.end(), it->first.data, it->first.data + it->first.bytesize());
            keys.off.push_back(keys.bytes.size());
            values.push_back(&it->second);
            const int n = (int)it->first.n();  // the loaded model's range of sizes holds its skipgrams (the reference never resets it in place, :889-891)
            if (n > maxn) maxn = n;
            if (n < minn) minn = n;
        }
        uint64_t   found   = 0;
        const auto t0      = std::chrono::steady_clock::now();
        const bool had     = hasskipgrams_;
        const bool corpus  = reverseindex != NULL && !reverseindex->empty();
        const bool indexed = colibri_host::is_indexed_value<ValueType>::value;
        if (values.empty()) {
            // nothing to look for
        } else if (colibri_host::recount_mode() == colibri_host::REPORT_HOST) {
            if (!corpus) {
                std::cerr << "ERROR: COLIBRI_RECOUNT=host needs the corpus attached to the model (its reverse index)" << std::endl;
                throw InternalError();
            }
            hasskipgrams_   = true;
            skipmasks_size_ = (size_t)-1;  // (the masks of the skipgrams just gathered)
            std::vector<PatternPointer> v;
            const unsigned int          ns = reverseindex->sentences();
            for (unsigned int s = 1; s <= ns; ++s) {
                const unsigned int sl = reverseindex->sentencelength((int)s);
                for (unsigned int t = 0; t < sl; ++t) {
                    v.clear();
                    reverseindex_ordered(IndexReference(s, (uint16_t)t), 0, SKIPGRAM, 0, v);
                    for (const PatternPointer& pp : v) {
                        valuehandler.add(getdata(Pattern(pp), true), IndexReference(s - 1 + firstsentence, (uint16_t)t));
                        ++found;
                    }
                }
            }
        } else {
            if (!device && !corpus) {
                std::cerr << "ERROR: trainskipgrams_selfconstrained needs the corpus: attached to the model (its reverse index), or still on the device after train()" << std::endl;
                throw InternalError();
            }
            colibri_host::TrainResult rr;
            const bool resident = colibri_host::device_recount(device, corpus ? reverseindex->beginpointer() : NULL, corpus ? reverseindex->bytesize() : 0, firstsentence, keys, indexed,
                                                               (uint32_t)options.MINTOKENS, rr);
            std::cerr << "(skipgram recount on the device: " << (resident ? "resident" : "uploaded") << " corpus)" << std::endl;
            for (size_t j = 0; j < values.size(); ++j) {
                colibri_host::value_from_result(rr, j, *values[j]);
                found += rr.counts[j];
            }
        }
        if (!values.empty() && std::getenv("COLIBRI_HOST_TIMING") != NULL)  // (with device_train's line: where the call's wall time goes)
            std::cerr << "COLIBRI_HOST_TIMING recount " << std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() << " ms on the "
                      << (colibri_host::recount_mode() == colibri_host::REPORT_HOST ? "host" : "device") << ", " << values.size() << " skipgrams, " << found << " occurrences" << std::endl;
        if (!found) {
            hasskipgrams_ = had;
            std::cerr << " None found" << std::endl;
        } else {
            hasskipgrams_ = found > 1;  // (as the reference writes it, :1595)
            if (!options.QUIET) std::cerr << " Found " << found << " skipgrams, 0 flexgrams ...";
        }
        const unsigned int pruned = this->prune(options.MINTOKENS);
        if (!options.QUIET) std::cerr << " pruned " << pruned << std::endl;
    }

    /** train(..., continued = true) on a model that holds patterns (reference :983-995, colibri-patternmodeller -E): the orders the model already has n-grams
     *  of are skipped, the others are counted on the device with a look-back that finds the loaded patterns (colibri_set_continuation); the new patterns
     *  join the map, the totals stay the model's (:1047-1048 and :1197 are guarded by !continued). */
    void train_continued(std::istream* in, const PatternModelOptions& options, uint32_t firstsentence) {
        this->materialise();  // (a model trained a moment ago: its patterns into the map first)
        if (options.DOSKIPGRAMS || options.DOSKIPGRAMS_EXHAUSTIVE || options.MINTOKENS < 2 || options.MINLENGTH > 1 || options.DOPATTERNPERLINE ||
            options.MAXBACKOFFLENGTH < options.MAXLENGTH || options.MINTOKENS_UNIGRAMS > options.MINTOKENS) {
            std::cerr << "ERROR: continued training is on the MI355X-accelerated path for MINTOKENS >= 2, MINLENGTH = 1, without skipgrams, back-off length, word threshold or "
                         "pattern list" << std::endl;
            throw InternalError();
        }
        if (!options.QUIET) std::cerr << "Continuing training on preloaded model, computing statistics..." << std::endl;
        colibri_host::ConstraintKeys known;
        known.off.push_back(0);
        for (typename MapType::iterator it = this->data.begin(); it != this->data.end(); ++it) {
            if (it->first.category() != NGRAM) continue;
            known.bytes.insert(known.bytes.end(), it->first.data, it->first.data + it->first.bytesize());
            known.off.push_back(known.bytes.size());
        }
        colibri_options o{};
        o.mintokens           = options.MINTOKENS;
        o.maxlength           = options.MAXLENGTH;
        o.minlength           = 1;
        o.maxbackofflength    = options.MAXBACKOFFLENGTH;
        o.mintokens_unigrams  = options.MINTOKENS_UNIGRAMS;
        o.mintokens_skipgrams = options.MINTOKENS_SKIPGRAMS;
        o.minskiptypes        = options.MINSKIPTYPES;
        o.maxskips            = options.MAXSKIPS;
        o.indexed             = colibri_host::is_indexed_value<ValueType>::value ? 1 : 0;
        colibri_host::TrainResult r;
        if (reverseindex != NULL && !reverseindex->empty()) {
            colibri_host::device_train(reverseindex->beginpointer(), reverseindex->bytesize(), o, firstsentence, r, &known, false, /*continuation=*/true);
        } else if (in != NULL) {
            const std::vector<unsigned char> payload = colibri_host::read_corpus_payload(*in);
            if (payload.empty()) {
                std::cerr << "ERROR: Attempting to read pattern from file, but file is empty?" << std::endl;
                throw InternalError();
            }
            colibri_host::device_train(payload.data(), payload.size(), o, firstsentence, r, &known, false, /*continuation=*/true);
        } else {
            std::cerr << "ERROR: No input stream and no reverse index (preloaded corpus) to train on" << std::endl;
            throw InternalError();
        }
        if (!options.QUIET) colibri_host::print_training_log(r.stats, o, std::cerr);
        for (size_t j = 0; j < r.size(); ++j) {
            ValueType v{};
            colibri_host::value_from_result(r, j, v);
            this->data[Pattern(r.key_bytes.data() + r.key_off[j], (size_t)(r.key_off[j + 1] - r.key_off[j]))] = std::move(v);
        }
        if (r.stats.npatterns && r.stats.maxn > maxn) maxn = r.stats.maxn;
        for (int n = 1; n < COLIBRI_MAX_ORDER; ++n)
            if (r.stats.kept[n] && n < minn) minn = n;
    }

    /** train(..., continued = false) on a model that holds patterns (reference :880-1270; colibri-patternmodeller -i model -f corpus -e N): the model is EXPANDED on
     *  different corpus data. Its n-grams and their counts seed the device run (colibri_set_seed): every order counts the corpus' windows whose sub-windows the
     *  model holds as it stands, adds the loaded counts, stops before the prune at the first order that creates no pattern, and otherwise prunes the order —
     *  loaded patterns included — by the summed counts. The merge (expand_merge.h): counts replaced by the sums, the corpus' references joined to the loaded ones,
     *  created patterns inserted, the loaded patterns that do not stay erased. totaltokens grows by the corpus'; totaltypes = the whole model's size at order 1
     *  (:1199-1201), untouched when the run stops there. The corpus is numbered from `firstsentence` throughout. */
    void train_expand(std::istream* in, const PatternModelOptions& options, uint32_t firstsentence) {
        this->materialise();  // (a model trained a moment ago: its patterns into the map first)
        if (options.DOSKIPGRAMS || options.DOSKIPGRAMS_EXHAUSTIVE || options.MINTOKENS < 2 || options.MINLENGTH > 1 || options.DOPATTERNPERLINE ||
            options.MAXBACKOFFLENGTH < options.MAXLENGTH || options.MINTOKENS_UNIGRAMS > options.MINTOKENS) {
            std::cerr << "ERROR: expanding a loaded model (train() on a non-empty model) is on the MI355X-accelerated path for MINTOKENS >= 2, MINLENGTH = 1, without skipgrams, "
                         "back-off length, word threshold or pattern list" << std::endl;
            throw InternalError();
        }
        if (colibri_host::gpus() > 1) {
            std::cerr << "ERROR: expanding a loaded model runs on one GPU (no --gpus)" << std::endl;
            throw InternalError();
        }
        if (!options.QUIET) std::cerr << "Training patternmodel on a loaded model (" << this->data.size() << " patterns), occurrence threshold: " << options.MINTOKENS << std::endl;
        colibri_host::ConstraintKeys               keys;
        colibri_host::SeedSet                      seed;
        std::vector<typename MapType::iterator>    its;
        keys.off.push_back(0);
        for (typename MapType::iterator it = this->data.begin(); it != this->data.end(); ++it) {
            if (it->first.category() != NGRAM) {
                std::cerr << "ERROR: the loaded model holds skipgrams or flexgrams: every order's prune would judge them too, and expanding does not count them on the "
                             "MI355X-accelerated path" << std::endl;
                throw InternalError();
            }
            keys.bytes.insert(keys.bytes.end(), it->first.data, it->first.data + it->first.bytesize());
            keys.off.push_back(keys.bytes.size());
            seed.counts.push_back((uint32_t)valuehandler.count(it->second));
            its.push_back(it);
        }
        colibri_options o{};
        o.mintokens           = options.MINTOKENS;
        o.maxlength           = options.MAXLENGTH;
        o.minlength           = 1;
        o.maxbackofflength    = options.MAXBACKOFFLENGTH;
        o.mintokens_unigrams  = options.MINTOKENS_UNIGRAMS;
        o.mintokens_skipgrams = options.MINTOKENS_SKIPGRAMS;
        o.minskiptypes        = options.MINSKIPTYPES;
        o.maxskips            = options.MAXSKIPS;
        o.indexed             = colibri_host::is_indexed_value<ValueType>::value ? 1 : 0;
        colibri_host::TrainResult r;
        if (reverseindex != NULL && !reverseindex->empty()) {
            colibri_host::device_train(reverseindex->beginpointer(), reverseindex->bytesize(), o, firstsentence, r, &keys, false, false, false, &seed);
        } else if (in != NULL) {
            const std::vector<unsigned char> payload = colibri_host::read_corpus_payload(*in);
            if (payload.empty()) {
                std::cerr << "ERROR: Attempting to read pattern from file, but file is empty?" << std::endl;
                throw InternalError();
            }
            colibri_host::device_train(payload.data(), payload.size(), o, firstsentence, r, &keys, false, false, false, &seed);
        } else {
            std::cerr << "ERROR: No input stream and no reverse index (preloaded corpus) to train on" << std::endl;
            throw InternalError();
        }
        if (!options.QUIET) colibri_host::print_training_log(r.stats, o, std::cerr);
        const size_t loaded = this->data.size();
        const colibri_host::ExpandMergeCounts n = colibri_host::expand_merge(
            this->data, its, seed.row, seed.kept, r.size(), [&](typename MapType::iterator it, size_t row) { expand_value(it->second, r, row); },
            [&](size_t row) {
                ValueType v{};
                colibri_host::value_from_result(r, row, v);
                this->data[Pattern(r.key_bytes.data() + r.key_off[row], (size_t)(r.key_off[row + 1] - r.key_off[row]))] = std::move(v);
            });
        expand_settle();
        if (!options.QUIET) std::cerr << " (" << n.merged << " loaded patterns counted again, " << n.created << " created, " << n.erased << " erased)" << std::endl;
        totaltokens += r.stats.totaltokens;
        if (r.stats.maxn >= 1) {
            totaltypes = loaded + r.stats.found[1];
            if (r.stats.maxn > maxn) maxn = r.stats.maxn;
            if (1 < minn) minn = 1;
        }
        trained_firstsentence_ = firstsentence;
    }
    // a loaded pattern's value after the run: the summed count; the corpus' references joined to its own
    static void expand_value(uint32_t& v, const colibri_host::TrainResult& r, size_t row) { v = r.counts[row]; }
    static void expand_value(IndexedData& v, const colibri_host::TrainResult& r, size_t row) {
        std::vector<IndexReference> fresh;
        for (uint64_t k = r.ref_off[row]; k < r.ref_off[row + 1]; ++k) fresh.push_back(IndexReference(r.ref_sentence[k], r.ref_token[k]));
        colibri_host::expand_join_refs(v.data, fresh.begin(), fresh.end());
    }
    // every list in ascending order when the run ends, as IndexedPatternModel::posttrain leaves them (reference :2699-2705)
    void expand_settle() { expand_settle_values((ValueType*)NULL); }
    void expand_settle_values(const uint32_t*) {}
    void expand_settle_values(const IndexedData*) {
        for (typename MapType::iterator it = this->data.begin(); it != this->data.end(); ++it) expand_sort(it->second);
    }
    static void expand_sort(uint32_t&) {}
    static void expand_sort(IndexedData& v) {
        if (!std::is_sorted(v.data.begin(), v.data.end())) std::sort(v.data.begin(), v.data.end());
    }

  public:
    /** erase the patterns of _n tokens (0 = any) that are not / are in the set (reference :2194-2242) */
    unsigned int prunenotinset(const std::unordered_set<Pattern>& s, int _n) { return prune_set(s, _n, false); }
    unsigned int pruneinset(const std::unordered_set<Pattern>& s, int _n) { return prune_set(s, _n, true); }

  protected:
    unsigned int prune_set(const std::unordered_set<Pattern>& s, int _n, bool erase_members) {
        unsigned int pruned = 0;
        if (s.empty()) return pruned;
        for (typename MapType::iterator it = this->begin(); it != this->end();) {
            if ((_n == 0 || (int)it->first.n() == _n) && ((s.find(it->first) != s.end()) == erase_members)) {
                it = this->data.erase(it);
                ++pruned;
            } else {
                ++it;
            }
        }
        return pruned;
    }
    /** the (n-1)-token sub-patterns of every pattern of n tokens */
    void subsumed_by(int n, std::unordered_set<Pattern>& out) {
        for (typename MapType::iterator it = this->begin(); it != this->end(); ++it) {
            if ((int)it->first.n() != n) continue;
            std::vector<std::string> toks;
            colibri_host::token_slices(it->first.data, it->first.bytesize(), toks);
            for (int first = 0; first + (n - 1) <= n; ++first) {
                std::string sub;
                for (int k = first; k < first + n - 1; ++k) sub += toks[(size_t)k];
                out.insert(Pattern((const unsigned char*)sub.data(), sub.size()));
            }
        }
    }
    /** PRUNENONSUBSUMED: from the longest patterns down, drop the (n-1)-grams no n-gram contains; PRUNESUBSUMED: from the shortest up, drop the
     *  (n-1)-grams some n-gram contains (reference :1280-1330). Post-hoc passes over the finished model, on the host. */
    void prune_by_subsumption(const PatternModelOptions& options) {
        if (options.PRUNENONSUBSUMED) {
            if (!options.QUIET) std::cerr << "Pruning non-subsumed n-grams" << std::endl;
            for (int n = std::min(options.PRUNENONSUBSUMED, options.MAXLENGTH); n > 1; n--) {
                std::unordered_set<Pattern> subsumed;
                subsumed_by(n, subsumed);
                const unsigned int k = prunenotinset(subsumed, n - 1);
                if (!options.QUIET) std::cerr << " pruned " << k << " non-subsumed " << (n - 1) << "-grams" << std::endl;
            }
        }
        if (options.PRUNESUBSUMED) {
            if (!options.QUIET) std::cerr << "Pruning subsumed n-grams" << std::endl;
            for (int n = 2; n <= std::min(options.PRUNESUBSUMED, options.MAXLENGTH); ++n) {
                std::unordered_set<Pattern> subsumed;
                subsumed_by(n, subsumed);
                const unsigned int k = pruneinset(subsumed, n - 1);
                if (!options.QUIET) std::cerr << " pruned " << k << " subsumed " << (n - 1) << "-grams" << std::endl;
            }
        }
    }

    /** the same two passes on the device (colibri_subsume, csrc/subsume.hpp), over the flat arrays of a run that train() has not installed yet: the model
     *  where it still lies in HBM, else its keys uploaded (a run over several GPUs, a constrained or a filtered one); then one pass over the arrays
     *  (keep_patterns) and the host route's lines from the fetched counts. false = nothing done, the host route has to (COLIBRI_SUBSUME, subsume_mode()). */
    bool prune_by_subsumption_on_device(colibri_host::TrainResult& r, const PatternModelOptions& options) {
        const colibri_host::ReportMode mode = colibri_host::subsume_mode();
        if (mode == colibri_host::REPORT_HOST) return false;
        const bool loud = mode == colibri_host::REPORT_DEVICE;
        if (!loud && r.size() < colibri_host::subsume_min_patterns()) return false;
        std::vector<uint8_t> keep;
        uint64_t             non[COLIBRI_MAX_ORDER] = {0}, sub[COLIBRI_MAX_ORDER] = {0};
        const int            p = options.PRUNENONSUBSUMED, S = options.PRUNESUBSUMED, l = options.MAXLENGTH;
        const bool resident = r.device && colibri_host::device_subsume_resident(r.device, r, p, S, l, loud, keep, non, sub);
        if (!resident && !colibri_host::device_subsume(r.key_off.data(), r.key_bytes.data(), r.size(), p, S, l, loud, keep, non, sub)) return false;
        if (loud) std::cerr << "(subsumption prune on the device: " << (resident ? "resident" : "uploaded") << " model)" << std::endl;
        colibri_host::keep_patterns(r, keep.data());
        auto count = [](const uint64_t* a, int tokens) { return tokens < COLIBRI_MAX_ORDER ? a[tokens] : 0; };  // (beyond the longest pattern nothing is pruned)
        if (p) {
            if (!options.QUIET) std::cerr << "Pruning non-subsumed n-grams" << std::endl;
            for (int n = std::min(p, l); n > 1 && !options.QUIET; n--) std::cerr << " pruned " << count(non, n - 1) << " non-subsumed " << (n - 1) << "-grams" << std::endl;
        }
        if (S) {
            if (!options.QUIET) std::cerr << "Pruning subsumed n-grams" << std::endl;
            for (int n = 2; n <= std::min(S, l) && !options.QUIET; ++n) std::cerr << " pruned " << count(sub, n - 1) << " subsumed " << (n - 1) << "-grams" << std::endl;
        }
        return true;
    }

  public:

    /** same, from a file name (reference :1353-1364); `.bz2` corpora are not accepted by this build */
    virtual void train(const std::string& filename, const PatternModelOptions& options, PatternModelInterface* constrainbymodel = NULL, PatternSet<>* filter = NULL,
                       bool continued = false, uint32_t firstsentence = 1, bool ignoreerrors = false) {
        if (filename.size() > 3 && filename.substr(filename.size() - 3) == ".bz2") {
            std::cerr << "ERROR: bz2-compressed corpora are not supported by this build; decompress first" << std::endl;
            throw InternalError();
        }
        std::ifstream in(filename, std::ios::in | std::ios::binary);
        if (!in.good() && !(reverseindex != NULL && !reverseindex->empty())) {
            std::cerr << "ERROR: Supplied data file can not be opened. Check whether it exists and whether you have proper permissions..." << std::endl;
            throw InternalError();
        }
        this->train(&in, options, constrainbymodel, filter, continued, firstsentence, ignoreerrors);
    }

    /** .colibri.patternmodel reader (reference :781-861 + PatternMapStore::read include/patternstore.h:555-619) */
    virtual void load(std::istream& f, const PatternModelOptions& options, PatternModelInterface* constrainmodel = NULL) {
        char null = 1;
        f.read(&null, 1);
        f.read((char*)&model_type, 1);
        f.read((char*)&model_version, 1);
        if (null != 0 || (model_type != UNINDEXEDPATTERNMODEL && model_type != INDEXEDPATTERNMODEL)) {
            std::cerr << "File is not a colibri model file (or a very old one, or a pointer/alignment model which this build does not read)" << std::endl;
            throw InternalError();
        }
        const unsigned char classencodingversion = model_version == 1 ? 1 : 2;
        f.read((char*)&totaltokens, sizeof(uint64_t));
        f.read((char*)&totaltypes, sizeof(uint64_t));
        uint64_t s = 0;
        f.read((char*)&s, sizeof(uint64_t));
        int mintokens = options.MINTOKENS == -1 ? 0 : options.MINTOKENS;
        this->data.clear();
        result.reset();
        flatindex.reset();
        this->pending_fill = nullptr;
        this->pending_size = nullptr;
        const bool file_indexed = model_type == INDEXEDPATTERNMODEL;
        for (uint64_t i = 0; i < s; ++i) {
            Pattern p = colibri_host::read_model_pattern(f, classencodingversion);
            ValueType value{};
            unsigned int cnt = 0;
            if (file_indexed) {
                IndexedData d;
                IndexedDataHandler().read(f, d);
                cnt = d.count();
                assign_loaded(value, d, cnt);
            } else {
                uint32_t c = 0;
                f.read((char*)&c, sizeof(uint32_t));
                cnt = c;
                IndexedData none;
                assign_loaded(value, none, c);
            }
            if (!f.good() && !f.eof()) {
                std::cerr << "ERROR: Exception occurred at pattern " << (i + 1) << " of " << s << std::endl;
                throw InternalError();
            }
            const PatternCategory c = p.category();
            if ((options.DOREMOVENGRAMS && c == NGRAM) || (options.DOREMOVESKIPGRAMS && c == SKIPGRAM) || (options.DOREMOVEFLEXGRAMS && c == FLEXGRAM)) continue;
            const int n = (int)p.n();
            if (n < options.MINLENGTH || n > options.MAXLENGTH) continue;
            if (cnt < (unsigned int)mintokens) continue;
            if (constrainmodel != NULL && !constrainmodel->has(p)) continue;
            if (options.DORESET) value = ValueType{};
            this->data[p] = value;
        }
        model_type    = (unsigned char)this->getmodeltype();
        model_version = 2;
        postread(options);
    }
    void load(const std::string& filename, const PatternModelOptions& options, PatternModelInterface* constrainmodel = NULL) {
        std::ifstream in(filename, std::ios::in | std::ios::binary);
        if (!in.good()) {
            std::cerr << "ERROR: Unable to load file " << filename << std::endl;
            throw InternalError();
        }
        this->load(in, options, constrainmodel);
    }
    /** recompute maxn / minn / hasskipgrams after loading (reference :572-588) */
    void postread(const PatternModelOptions&) {
        maxn = 0;
        minn = 999;
        for (typename MapType::iterator it = this->begin(); it != this->end(); ++it) {
            const int n = (int)it->first.n();
            if (n > maxn) maxn = n;
            if (n < minn) minn = n;
            if (!hasskipgrams_ && it->first.category() == SKIPGRAM) hasskipgrams_ = true;
        }
    }

    /** .colibri.patternmodel writer (reference :1609-1632, include/patternstore.h:534-542): 00, type, version 2, u64 tokens,
     *  u64 types, u64 npatterns, then per pattern: key bytes, 00, value. Streams straight from the device export when the map
     *  has not been materialised. */
    void write(std::ostream& out) {
        const char          null = 0;
        const unsigned char t = (unsigned char)this->getmodeltype(), v = 2;
        out.write(&null, 1);
        out.write((const char*)&t, 1);
        out.write((const char*)&v, 1);
        out.write((const char*)&totaltokens, sizeof(uint64_t));
        const uint64_t tp = this->types();
        out.write((const char*)&tp, sizeof(uint64_t));
        const uint64_t s = (uint64_t)this->size();
        out.write((const char*)&s, sizeof(uint64_t));
        if (result) {
            const colibri_host::TrainResult& r = *result;
            for (size_t j = 0; j < r.size(); ++j) {
                out.write((const char*)r.key_bytes.data() + r.key_off[j], (std::streamsize)(r.key_off[j + 1] - r.key_off[j]));
                out.write(&null, 1);
                colibri_host::write_value_from_result(out, r, j, (const ValueType*)NULL);
            }
        } else {
            for (typename MapType::iterator it = this->begin(); it != this->end(); ++it) {
                it->first.write(out);
                valuehandler.write(out, it->second);
            }
        }
    }
    void write(const std::string& filename) {
        std::ofstream out(filename, std::ios::out | std::ios::binary);
        this->write(out);
    }

    // ---- views: print / report / histogram, text-identical to the reference's (goldens: tests/golden/views/) --------------------------------

    /** statistics per (category, size) group, 0 = all (reference computestats :1903-1935): occurrences and distinct patterns */
    void computestats() {
        if (stats_from_device(false)) return;
        computestats_host();
    }
    void computestats_host() {
        cache_categories.clear();
        cache_n.clear();
        cache_grouptotal.clear();
        cache_grouptotalpatterns.clear();
        cache_categories.insert(0);
        cache_n.insert(0);
        for (typename MapType::iterator it = this->begin(); it != this->end(); ++it) {
            const int          c   = (int)it->first.category();
            const int          n   = (int)it->first.n();
            const unsigned int occ = valuehandler.count(it->second);
            cache_categories.insert(c);
            cache_n.insert(n);
            const int cs[2] = {c, 0}, ns[2] = {n, 0};
            for (int ci = 0; ci < 2; ++ci)
                for (int ni = 0; ni < 2; ++ni) {
                    if (ni == 0 && c == FLEXGRAM) continue;  // flexgrams have no per-size rows (:1918)
                    cache_grouptotal[cs[ci]][ns[ni]] += occ;
                    cache_grouptotalpatterns[cs[ci]][ns[ni]] += 1;
                }
        }
    }
    virtual void resetstats() {
        cache_grouptotalwordtypes.clear();
        cache_grouptotaltokens.clear();
        cache_coverage_done = false;
    }
    /**
     * word types and covered tokens per group (reference computecoveragestats :1946-1995). The reference walks the whole model once per group;
     * here every pattern is visited once and dropped into the (at most four) groups it belongs to. A group's word types are the distinct
     * tokens of its patterns — a skipgram's gap counts as one type, as it does there (pattern.ngrams(…,1) yields the gap token).
     * Unindexed models: the "covered tokens" of every group is the occurrence total of the whole model (the reference adds each pattern's count
     * outside its group filter, :1974), capped to tokens() by report().
     */
    virtual void computecoveragestats(int category = 0, int n = 0) {
        (void)category;
        (void)n;
        if (cache_coverage_done || this->size() == 0) return;
        if (stats_from_device(true)) {
            cache_coverage_done = true;
            return;
        }
        if (cache_grouptotal.empty()) computestats_host();
        std::map<int, std::map<int, std::unordered_set<std::string>>> typesets;
        uint64_t alloccurrences = 0;
        for (typename MapType::iterator it = this->begin(); it != this->end(); ++it) {
            const int c = (int)it->first.category(), pn = (int)it->first.n();
            alloccurrences += valuehandler.count(it->second);
            std::vector<std::string> toks;
            colibri_host::token_slices(it->first.data, it->first.bytesize(), toks);
            const int cs[2] = {c, 0}, ns[2] = {pn, 0};
            for (int ci = 0; ci < 2; ++ci)
                for (int ni = 0; ni < 2; ++ni)
                    for (const std::string& t : toks) typesets[cs[ci]][ns[ni]].insert(t);
            this->coverage_visit(it, c, pn);
        }
        for (const int c : cache_categories)
            for (const int gn : cache_n) {
                cache_grouptotalwordtypes[c][gn] = (unsigned int)typesets[c][gn].size();
                cache_grouptotaltokens[c][gn]    = this->coverage_tokens(c, gn, alloccurrences);
            }
        this->coverage_finish();
        cache_coverage_done = true;
    }
    /**
     * computestats() (coverage = false) or computecoveragestats() from one device call (colibri_coverage, csrc/coverage.hpp): the caches get what the
     * host loops would have put there, the reference's quirks applied here. A model fresh from the device goes up as its flat arrays — or is read
     * where it still lies in HBM — without being materialised. false = nothing done, the host path has to (COLIBRI_REPORT, report_mode()).
     */
    bool stats_from_device(bool coverage) {
        const colibri_host::ReportMode mode = colibri_host::report_mode();
        if (mode == colibri_host::REPORT_HOST || this->size() == 0) return false;
        const bool     loud    = mode == colibri_host::REPORT_DEVICE;
        const bool     indexed = colibri_host::is_indexed_value<ValueType>::value;
        const uint64_t minwork = colibri_host::report_min_work();
        colibri_host::CoverageGroups g;
        bool done = false, resident = false;
        if (result) {
            const colibri_host::TrainResult& r = *result;
            if (indexed && r.ref_off.empty()) return false;  // (an unindexed result under an indexed model: every count is 0 — left to the host path)
            if (!loud && r.size() + (indexed ? r.ref_sentence.size() : 0) < minwork) return false;
            if (r.device) done = resident = colibri_host::device_coverage_resident(r.device, r, coverage, loud, g);
            if (!done)
                done = colibri_host::device_coverage(r.key_off.data(), r.key_bytes.data(), indexed ? NULL : r.counts.data(), indexed ? r.ref_off.data() : NULL,
                                                     indexed ? r.ref_sentence.data() : NULL, indexed ? r.ref_token.data() : NULL, r.size(), coverage, loud, g);
        } else {
            std::vector<uint64_t>      key_off(1, 0), ref_off(1, 0);
            std::vector<unsigned char> key_bytes;
            std::vector<uint32_t>      counts, rs;
            std::vector<uint16_t>      rt;
            if (!loud) {
                uint64_t work = this->size();
                for (typename MapType::iterator it = this->begin(); indexed && it != this->end() && work < minwork; ++it) work += valuehandler.count(it->second);
                if (work < minwork) return false;
            }
            for (typename MapType::iterator it = this->begin(); it != this->end(); ++it) {
                key_bytes.insert(key_bytes.end(), it->first.data, it->first.data + it->first.bytesize());
                key_off.push_back(key_bytes.size());
                if (indexed) {
                    flatten_refs(it->second, rs, rt);
                    ref_off.push_back(rs.size());
                } else {
                    counts.push_back(valuehandler.count(it->second));
                }
            }
            rs.push_back(0);
            rt.push_back(0);
            done = colibri_host::device_coverage(key_off.data(), key_bytes.data(), indexed ? NULL : counts.data(), indexed ? ref_off.data() : NULL, indexed ? rs.data() : NULL,
                                                 indexed ? rt.data() : NULL, this->size(), coverage, loud, g);
        }
        if (!done) return false;
        if (loud) std::cerr << "(statistics on the device: " << (resident ? "resident" : "uploaded") << " model)" << std::endl;
        const size_t G = g.G;
        cache_categories.clear();
        cache_n.clear();
        cache_grouptotal.clear();
        cache_grouptotalpatterns.clear();
        cache_categories.insert(0);
        cache_n.insert(0);
        for (size_t c = 1; c < 4; ++c)
            if (g.patterns[c * G]) cache_categories.insert((int)c);
        for (size_t n = 1; n < G; ++n)
            if (g.types[n]) cache_n.insert((int)n);  // (a size only flexgrams have has types, but no patterns: computestats gives flexgrams no per-size rows)
        for (size_t c = 0; c < 4; ++c)
            for (size_t n = 0; n < G; ++n)
                if (g.patterns[c * G + n]) {
                    cache_grouptotal[(int)c][(int)n]         = g.counts[c * G + n];
                    cache_grouptotalpatterns[(int)c][(int)n] = g.patterns[c * G + n];
                }
        if (!coverage) return true;
        for (const int c : cache_categories)
            for (const int gn : cache_n) {
                cache_grouptotalwordtypes[c][gn] = (unsigned int)g.types[(size_t)c * G + gn];
                // indexed: the reference fills only the all-sizes rows; unindexed: every group gets the occurrences of the whole model (computecoveragestats above)
                cache_grouptotaltokens[c][gn] = indexed ? (gn != 0 ? 0 : g.tokens[(size_t)c * G]) : g.counts[0];
            }
        return true;
    }
    unsigned int totaloccurrencesingroup(int category, int n) {
        if (cache_grouptotal.empty() && this->size() != 0) computestats();
        return (unsigned int)cache_grouptotal[category][n];
    }
    unsigned int totalpatternsingroup(int category, int n) {
        if (cache_grouptotalpatterns.empty() && this->size() != 0) computestats();
        return (unsigned int)cache_grouptotalpatterns[category][n];
    }
    unsigned int totalwordtypesingroup(int category, int n) {
        if (cache_grouptotalwordtypes.empty() && this->size() != 0) computecoveragestats(category, n);
        return cache_grouptotalwordtypes[category][n];
    }
    unsigned int totaltokensingroup(int category, int n) {
        if (cache_grouptotaltokens.empty() && this->size() != 0) computecoveragestats(category, n);
        return (unsigned int)cache_grouptotaltokens[category][n];
    }
    /** occurrences × size: a maximal projection, also for indexed models (reference :1725-1727) */
    size_t coveragecount(const Pattern& key) { return (size_t)this->occurrencecount(key) * key.size(); }
    double coverage(const Pattern& key) { return coveragecount(key) / (double)this->tokens(); }

    /** the whole model, one pattern per line, under the reference's header (reference :2294-2321; the legend goes to stderr there and here) */
    virtual void print(std::ostream& out, const ClassDecoder& decoder, bool instantiate = false) {
        instantiate = instantiate && instances_apply();
        if (print_from_device(out, decoder, instantiate)) return;  // (the device refuses what check_instances() refuses, before it hands a byte over)
        if (instantiate) check_instances();  // a flexgram, or a reference that does not fit the corpus: refused before the header
        instances_checked_ = instantiate;    // (the rows below need not look again)
        bool haveoutput = false;
        for (typename MapType::iterator it = this->begin(); it != this->end(); ++it) {
            if (!haveoutput) {
                out << "PATTERN\tCOUNT\tTOKENS\tCOVERAGE\tCATEGORY\tSIZE\tFREQUENCY" << (colibri_host::is_indexed_value<ValueType>::value ? "\tREFERENCES" : "") << std::endl;
                haveoutput = true;
            }
            this->print(out, decoder, it->first, instantiate, true);
        }
        instances_checked_ = false;
        if (haveoutput) colibri_host::print_legend(std::cerr, colibri_host::is_indexed_value<ValueType>::value);
    }
    /**
     * The model in export layout for a device call, without materialising a model fresh from the device: `result`'s arrays as they are, or the map
     * flattened as outputrelations_model flattens it. refs = false: the references themselves are not needed. false = under `minwork` patterns + references.
     */
    struct FlatView {
        std::vector<uint64_t>      key_off, ref_off;
        std::vector<unsigned char> key_bytes;
        std::vector<uint32_t>      counts, rs;
        std::vector<uint16_t>      rt;
        const uint64_t *           ko = NULL, *ro = NULL;
        const unsigned char*       kb = NULL;
        const uint32_t *           ct = NULL, *s = NULL;
        const uint16_t*            t = NULL;
        uint64_t                   np = 0;
    };
    bool flat_view(FlatView& v, bool refs, uint64_t minwork) {
        const bool indexed = colibri_host::is_indexed_value<ValueType>::value;
        if (result) {
            const colibri_host::TrainResult& r = *result;
            if (indexed && r.ref_off.empty()) return false;  // (an unindexed result under an indexed model: every count is 0 — left to the host path)
            if (r.size() + (indexed ? r.ref_sentence.size() : 0) < minwork) return false;
            v.np = r.size();
            v.ko = r.key_off.data();
            v.kb = r.key_bytes.data();
            v.ct = indexed ? NULL : r.counts.data();
            v.ro = indexed ? r.ref_off.data() : NULL;
            v.s  = indexed ? r.ref_sentence.data() : NULL;
            v.t  = indexed ? r.ref_token.data() : NULL;
            return true;
        }
        if (minwork) {
            uint64_t work = this->size();
            for (typename MapType::iterator it = this->begin(); indexed && it != this->end() && work < minwork; ++it) work += valuehandler.count(it->second);
            if (work < minwork) return false;
        }
        v.key_off.assign(1, 0);
        v.ref_off.assign(1, 0);
        for (typename MapType::iterator it = this->begin(); it != this->end(); ++it) {
            v.key_bytes.insert(v.key_bytes.end(), it->first.data, it->first.data + it->first.bytesize());
            v.key_off.push_back(v.key_bytes.size());
            if (indexed) {
                if (refs) {
                    flatten_refs(it->second, v.rs, v.rt);
                    v.ref_off.push_back(v.rs.size());
                } else {
                    v.ref_off.push_back(v.ref_off.back() + valuehandler.count(it->second));
                }
            } else {
                v.counts.push_back(valuehandler.count(it->second));
            }
        }
        v.key_bytes.push_back(0);
        v.rs.push_back(0);
        v.rt.push_back(0);
        v.counts.push_back(0);
        v.np = this->size();
        v.ko = v.key_off.data();
        v.kb = v.key_bytes.data();
        v.ct = indexed ? NULL : v.counts.data();
        v.ro = indexed ? v.ref_off.data() : NULL;
        v.s  = indexed ? v.rs.data() : NULL;
        v.t  = indexed ? v.rt.data() : NULL;
        return true;
    }
    /**
     * print() from one device call (colibri_print_model, csrc/print.hpp): the header here, the rows from the device in the order of the flat arrays,
     * the legend here. Only for a stream in its default float state (the rows are written for precision 6, no flags). false = nothing written, the host
     * loop has to (COLIBRI_PRINT, print_mode()).
     */
    bool print_from_device(std::ostream& out, const ClassDecoder& decoder, bool instantiate = false) {
        const colibri_host::ReportMode mode = colibri_host::print_mode();
        if (mode == colibri_host::REPORT_HOST || this->size() == 0) return false;
        const bool loud    = mode == colibri_host::REPORT_DEVICE;
        const bool indexed = colibri_host::is_indexed_value<ValueType>::value;
        if (!colibri_host::stream_in_default_float_state(out)) {
            if (loud) std::cerr << "ERROR: COLIBRI_PRINT=device, but the stream is not in its default float state (precision 6, no float flags, width 0): the host path prints" << std::endl;
            return false;
        }
        FlatView v;
        if (!flat_view(v, true, loud ? 0 : colibri_host::print_min_work())) {
            if (loud) std::cerr << "ERROR: COLIBRI_PRINT=device, but this model has no device form (an indexed model over unindexed results): the host path prints" << std::endl;
            return false;
        }
        // the header goes out first: the rows follow it on the same stream. Until the first row is written a refusal can still hand over to the host loop,
        // which writes its own header: so the rows are collected behind it only when the call is known to run — the device writes nothing before it has
        // every length, and refuses before that.
        std::ostringstream head;
        head << "PATTERN\tCOUNT\tTOKENS\tCOVERAGE\tCATEGORY\tSIZE\tFREQUENCY" << (indexed ? "\tREFERENCES" : "") << std::endl;
        struct HeaderFirst : std::streambuf {  // writes the header before the first piece of rows, and nothing if no piece ever comes
            std::ostream& o;
            std::string   h;
            bool          done = false;
            HeaderFirst(std::ostream& o_, const std::string& h_) : o(o_), h(h_) {}
            std::streamsize xsputn(const char* s, std::streamsize n) override {
                if (!done) {
                    o << h;
                    done = true;
                }
                o.write(s, n);
                return o.good() ? n : 0;
            }
            int overflow(int ch) override {
                if (ch == EOF) return 0;
                const char c = (char)ch;
                return xsputn(&c, 1) == 1 ? ch : EOF;
            }
        } buf(out, head.str());
        std::ostream rows(&buf);
        bool done = false, resident = false;
        // with instances the device reads the corpus: the resident form takes the context's own (the one the model was trained on, numbered as it was then),
        // the uploaded form uploads the attached one first
        if (result && result->device) done = resident = colibri_host::device_print_resident(result->device, *result, decoder.words(), this->tokens(), loud, rows, instantiate);
        if (!done)
            done = colibri_host::device_print(decoder.words(), v.ko, v.kb, v.ct, v.ro, v.s, v.t, v.np, this->tokens(), loud, rows, instantiate,
                                              instantiate ? reverseindex->beginpointer() : NULL, instantiate ? reverseindex->bytesize() : 0, trained_firstsentence_);
        if (!done) return false;
        out.flush();
        if (loud) std::cerr << "(print on the device: " << (resident ? "resident" : "uploaded") << " model" << (instantiate ? ", instances" : "") << ")" << std::endl;
        colibri_host::print_legend(std::cerr, indexed);
        return true;
    }
    /** histogram()'s (count, patterns) pairs from one device call (colibri_histogram); false = the host loop has to (COLIBRI_HISTOGRAM, histogram_mode()) */
    bool histogram_from_device(int category, unsigned int size, colibri_host::HistogramRows& rows) {
        const colibri_host::ReportMode mode = colibri_host::histogram_mode();
        if (mode == colibri_host::REPORT_HOST || this->size() == 0) return false;
        const bool loud = mode == colibri_host::REPORT_DEVICE;
        FlatView   v;
        if (!flat_view(v, false, loud ? 0 : colibri_host::print_min_work())) {
            if (loud) std::cerr << "ERROR: COLIBRI_HISTOGRAM=device, but this model has no device form (an indexed model over unindexed results): the host path counts" << std::endl;
            return false;
        }
        bool done = false, resident = false;
        if (result && result->device) done = resident = colibri_host::device_histogram_resident(result->device, *result, category, size, loud, rows);
        if (!done) done = colibri_host::device_histogram(v.ko, v.kb, v.ct, v.ro, v.np, category, size, loud, rows);
        if (!done) return false;
        if (loud) std::cerr << "(histogram on the device: " << (resident ? "resident" : "uploaded") << " model)" << std::endl;
        return true;
    }
    /** one pattern: text, count, count×size, that over tokens(), category, size, frequency within its (category, size) group (reference :2354-2373, :2930-2959) */
    void print(std::ostream& out, const ClassDecoder& decoder, const Pattern& pattern, bool instantiate = false, bool endline = true) {
        instantiate = instantiate && instances_apply() && pattern.category() != NGRAM;
        if (instantiate && !instances_checked_) {
            typename MapType::iterator found = this->find(pattern);
            if (found != this->end()) check_instances_of(found->first, found->second);  // (before the row's first byte)
        }
        const unsigned int count    = this->occurrencecount(pattern);
        const size_t       covcount = this->coveragecount(pattern);
        const int          cat      = (int)pattern.category();
        out << pattern.tostring(decoder) << "\t" << count << "\t" << covcount << "\t" << covcount / (double)this->tokens() << "\t"
            << (cat == NGRAM ? "ngram" : cat == SKIPGRAM ? "skipgram" : cat == FLEXGRAM ? "flexgram" : "") << "\t" << pattern.size() << "\t" << this->frequency(pattern);
        typename MapType::iterator it = this->find(pattern);
        if (it != this->end()) {
            if (instantiate) print_value_instances(out, decoder, it->second, (uint32_t)pattern.size());
            else print_value_extra(out, it->second);
        }
        if (endline) out << std::endl;
    }
    /** print(..., instantiate = true) writes instances: an indexed model with a corpus attached (reference :2952) */
    bool instances_apply() const { return colibri_host::is_indexed_value<ValueType>::value && reverseindex != NULL && !reverseindex->empty(); }
    /** the corpus text a pattern stands for at one of its references (reference :2667-2673: IndexedCorpus::findpattern) */
    PatternPointer getinstance(const IndexReference& begin, const PatternPointer& pattern) {
        if (reverseindex == NULL) {
            std::cerr << "ERROR: You must specify a reverse index to use getinstance()!" << std::endl;
            throw InternalError();
        }
        return reverseindex->findpattern(begin, Pattern(pattern));
    }
    void printpattern(std::ostream& out, const ClassDecoder& decoder, const Pattern& pattern, bool instantiate = false, bool endline = true) {
        this->print(out, decoder, pattern, instantiate, endline);
    }
    /** pointer-style call kept for callers of the earlier form of this face: the same table; hex keys when there is no decoder */
    void print(std::ostream* out, const ClassDecoder* decoder = NULL) {
        if (decoder != NULL) {
            this->print(*out, *decoder, false);
            return;
        }
        for (typename MapType::iterator it = this->begin(); it != this->end(); ++it) {
            *out << it->first.tohex() << "\t" << valuehandler.count(it->second);
            print_value_extra(*out, it->second);
            *out << std::endl;
        }
    }

    /** occurrence count -> number of patterns (reference :2391-2410). cap keeps the top counts until `cap` patterns are covered. */
    void histogram(std::map<unsigned int, unsigned int>& hist, unsigned int threshold = 0, unsigned int cap = 0, int category = 0, unsigned int size = 0) {
        colibri_host::HistogramRows rows;
        if (histogram_from_device(category, size, rows)) {
            for (size_t j = 0; j < rows.counts.size(); ++j)
                if (rows.counts[j] >= threshold) hist[rows.counts[j]] += (unsigned int)rows.patterns[j];
        } else {
            for (typename MapType::iterator it = this->begin(); it != this->end(); ++it) {
                if ((category != 0 && (int)it->first.category() != category) || (size != 0 && size != it->first.size())) continue;
                const unsigned int c = valuehandler.count(it->second);
                if (c >= threshold) hist[c]++;
            }
        }
        if (cap > 0) {
            unsigned int sum = 0;
            std::map<unsigned int, unsigned int>::iterator cut = hist.end();
            while (sum < cap && cut != hist.begin()) {
                --cut;
                sum += cut->second;
            }
            hist.erase(hist.begin(), cut);
        }
    }
    void histogram(std::ostream& OUT, unsigned int threshold = 0, unsigned int cap = 0, int category = 0, unsigned int size = 0) {  // reference :2432-2441
        std::map<unsigned int, unsigned int> hist;
        histogram(hist, threshold, cap, category, size);
        OUT << "HISTOGRAM" << std::endl << "------------------------------" << std::endl << "OCCURRENCES\tPATTERNS" << std::endl;
        for (const auto& kv : hist) OUT << kv.first << "\t" << kv.second << std::endl;
    }
    void histogram(std::ostream* out) { histogram(*out); }
    /** smallest occurrence count among the top `amount` patterns (reference :2412-2422) */
    unsigned int topthreshold(int amount, int category = 0, int size = 0) {
        std::map<unsigned int, unsigned int> hist;
        histogram(hist, 0, (unsigned int)amount, category, (unsigned int)size);
        return hist.empty() ? 0 : hist.begin()->first;
    }

    /** the REPORT table (reference :2499-2601): totals, coverage, then one row per (category, size) group; leaves OUT in fixed/4 like the reference */
    void report(std::ostream& OUT, bool nocoverage = false) {
        const bool indexed = this->getmodeltype() != UNINDEXEDPATTERNMODEL;
        if (this->size() != 0) {
            if (nocoverage) {
                std::cerr << "Computing statistics without coverage information..." << std::endl;
                computestats();
            } else {
                std::cerr << "Computing statistics with coverage information (may take a while)..." << std::endl;
                computecoveragestats();
            }
        }
        const int W = 15;
        OUT << std::setiosflags(std::ios::fixed) << std::setprecision(4) << std::endl;
        OUT << "REPORT" << std::endl;
        if (!indexed && !nocoverage) {
            OUT << "   Warning: Model is unindexed, token coverage counts are mere maximal projections" << std::endl;
            OUT << "            assuming no overlap at all!!! Use an indexed model for accurate coverage counts" << std::endl;
        }
        OUT << "----------------------------------" << std::endl;
        OUT << "                          " << std::setw(W) << "PATTERNS" << std::setw(W) << "TOKENS" << std::setw(W) << "COVERAGE" << std::setw(W) << "TYPES" << std::setw(W) << std::endl;
        OUT << "Total:                    " << std::setw(W) << "-" << std::setw(W) << this->tokens() << std::setw(W) << "-" << std::setw(W) << this->types() << std::endl;
        if (!nocoverage) {
            const size_t coveredtypes  = totalwordtypesingroup(0, 0);
            size_t       coveredtokens = totaltokensingroup(0, 0);
            if (coveredtokens > this->tokens()) coveredtokens = this->tokens();
            const size_t uncoveredtokens = this->tokens() - coveredtokens;
            OUT << "Uncovered:                " << std::setw(W) << "-" << std::setw(W) << uncoveredtokens << std::setw(W) << uncoveredtokens / (double)this->tokens() << std::setw(W)
                << this->types() - coveredtypes << std::endl;
            OUT << "Covered:                  " << std::setw(W) << this->size() << std::setw(W) << coveredtokens << std::setw(W) << coveredtokens / (double)this->tokens() << std::setw(W)
                << coveredtypes << std::endl
                << std::endl;
        } else {
            OUT << std::endl;
        }
        bool haveoutput = false;
        for (const int c : cache_categories) {
            if (!cache_grouptotalpatterns.count(c)) continue;
            for (const int n : cache_n) {
                if (!cache_grouptotalpatterns[c].count(n)) continue;
                if (!haveoutput) {
                    OUT << std::setw(W) << "CATEGORY" << std::setw(W) << "N (SIZE) " << std::setw(W) << "PATTERNS";
                    if (indexed && !nocoverage) OUT << std::setw(W) << "TOKENS" << std::setw(W) << "COVERAGE";
                    if (!nocoverage) OUT << std::setw(W) << "TYPES";
                    OUT << std::setw(W) << "OCCURRENCES" << std::endl;
                    haveoutput = true;
                }
                OUT << std::setw(W) << (c == 0 ? "all" : c == NGRAM ? "n-gram" : c == SKIPGRAM ? "skipgram" : "flexgram");
                if (n == 0) OUT << std::setw(W) << "all";
                else OUT << std::setw(W) << n;
                OUT << std::setw(W) << cache_grouptotalpatterns[c][n];
                if (indexed && !nocoverage) OUT << std::setw(W) << cache_grouptotaltokens[c][n] << std::setw(W) << cache_grouptotaltokens[c][n] / (double)this->tokens();
                if (!nocoverage) OUT << std::setw(W) << cache_grouptotalwordtypes[c][n];
                OUT << std::setw(W) << cache_grouptotal[c][n] << std::endl;
            }
        }
        if (haveoutput) colibri_host::report_legend(std::cerr, indexed);
    }
    void report(std::ostream* out, bool nocoverage = false) { report(*out, nocoverage); }

  protected:
    std::set<int>                                  cache_categories, cache_n;
    std::map<int, std::map<int, uint64_t>>         cache_grouptotal, cache_grouptotalpatterns, cache_grouptotaltokens;
    std::map<int, std::map<int, unsigned int>>     cache_grouptotalwordtypes;
    bool                                           cache_coverage_done = false;
    // hooks the indexed model fills in to count really covered positions (reference :3390-3450)
    virtual void     coverage_visit(typename MapType::iterator, int, int) {}
    virtual uint64_t coverage_tokens(int, int, uint64_t alloccurrences) { return alloccurrences; }
    virtual void     coverage_finish() {}

  private:
    static void assign_loaded(uint32_t& dst, const IndexedData&, unsigned int count) { dst = count; }
    static void assign_loaded(IndexedData& dst, const IndexedData& src, unsigned int) { dst = src; }  // unindexed file -> indexed model: patterns load, counts are lost (reference :837-841)
    static void flatten_refs(const uint32_t&, std::vector<uint32_t>&, std::vector<uint16_t>&) {}
    static void flatten_refs(const IndexedData& d, std::vector<uint32_t>& rs, std::vector<uint16_t>& rt) {
        for (const IndexReference& r : d.data) {
            rs.push_back(r.sentence);
            rt.push_back(r.token);
        }
    }
    // print() with instances (reference :2948-2959): what it refuses, it refuses before a byte is written. A flexgram: the reference's walk for it accepts gaps
    // of exactly one token and throws otherwise. A reference whose window is not in the corpus (a model beside another corpus): the reference aborts.
    void check_instances() {
        for (typename MapType::iterator it = this->begin(); it != this->end(); ++it) check_instances_of(it->first, it->second);
    }
    void check_instances_of(const Pattern&, const uint32_t&) {}
    void check_instances_of(const Pattern& pattern, const IndexedData& d) {
        const PatternCategory cat = pattern.category();
        if (cat == NGRAM) return;
        if (cat == FLEXGRAM) {
            std::cerr << "ERROR: print with instances: the model holds flexgrams, which are not instantiated (the reference's walk accepts gaps of exactly one token)" << std::endl;
            throw InternalError();
        }
        const uint32_t n = (uint32_t)pattern.size();
        PatternPointer w;
        for (const IndexReference& r : d.data)
            if (!reverseindex->instancewindow(trained_firstsentence_, r.sentence, r.token, n, w)) {
                std::cerr << "ERROR: print with instances: the reference " << r.tostring() << " of a skipgram of " << n << " tokens does not fit the corpus (is it the model's corpus?)"
                          << std::endl;
                throw KeyError();
            }
    }
    void print_value_instances(std::ostream&, const ClassDecoder&, const uint32_t&, uint32_t) {}
    void print_value_instances(std::ostream& out, const ClassDecoder& decoder, const IndexedData& d, uint32_t n) {
        out << "\t";
        bool first = true;
        for (const IndexReference& r : d.data) {
            if (!first) out << ' ';
            PatternPointer w;
            reverseindex->instancewindow(trained_firstsentence_, r.sentence, r.token, n, w);  // (it fits: check_instances_of)
            out << r.tostring() << '[' << colibri_host::decode_key(w.data, w.bytes, decoder) << ']';
            first = false;
        }
    }
    static void print_value_extra(std::ostream&, const uint32_t&) {}
    static void print_value_extra(std::ostream& out, const IndexedData& d) {
        out << "\t";
        bool first = true;
        for (const IndexReference& r : d.data) {
            if (!first) out << ' ';
            out << r.tostring();
            first = false;
        }
    }
};

/** The patterns of a model file as a set — what the reference loads a constraint model as (include/patternmodel.h:283-530; colibri-patternmodeller -j,
 *  src/patternmodeller.cpp:712-718). Here it is an unindexed model whose values are not looked at. */
class PatternSetModel : public PatternModel<uint32_t> {
  public:
    PatternSetModel() : PatternModel<uint32_t>() {}
    PatternSetModel(const std::string& filename, const PatternModelOptions& options, PatternModelInterface* constrainmodel = NULL) : PatternModel<uint32_t>(filename, options, constrainmodel) {}
    int getmodeltype() const override { return PATTERNSETMODEL; }
};

/** pattern -> relation count (reference include/patternmodel.h:220) */
typedef PatternMap<uint32_t> t_relationmap;
/** pattern -> relation value (reference include/patternmodel.h:221) */
typedef PatternMap<double> t_relationmap_double;

/** Indexed model: pattern -> sorted list of (sentence, token). reference include/patternmodel.h:2682-3875. */
template <class MapType = PatternMap<IndexedData>>
class IndexedPatternModel : public PatternModel<IndexedData, IndexedDataHandler, MapType> {
  public:
    IndexedPatternModel<MapType>(IndexedCorpus* corpus = NULL) : PatternModel<IndexedData, IndexedDataHandler, MapType>(corpus) {}
    IndexedPatternModel<MapType>(const std::string& filename, const PatternModelOptions& options, PatternModelInterface* constrainmodel = NULL, IndexedCorpus* corpus = NULL)
        : PatternModel<IndexedData, IndexedDataHandler, MapType>(filename, options, constrainmodel, corpus) {}
    int getmodeltype() const override { return INDEXEDPATTERNMODEL; }

  protected:
    // Really covered positions (reference :3390-3450): every occurrence covers size() consecutive positions, gaps included. The reference
    // fills this only for the "all sizes" rows — its per-size test compares the *argument* n (0 from report()) with the group's size
    // (:3425) — so per-size rows report 0 tokens there, and here.
    std::map<int, std::vector<uint64_t>> covered_;
    void coverage_visit(typename PatternMap<IndexedData>::iterator it, int c, int pn) override {
        std::vector<uint64_t>&bycat = covered_[c], &all = covered_[0];
        for (const IndexReference& r : it->second.data)
            for (int i = 0; i < pn; ++i) {
                const uint64_t pos = ((uint64_t)r.sentence << 16) | (uint16_t)(r.token + i);
                bycat.push_back(pos);
                all.push_back(pos);
            }
    }
    uint64_t coverage_tokens(int c, int gn, uint64_t) override {
        if (gn != 0) return 0;
        std::vector<uint64_t>& v = covered_[c];
        std::sort(v.begin(), v.end());
        return (uint64_t)(std::unique(v.begin(), v.end()) - v.begin());
    }
    void coverage_finish() override { covered_.clear(); }

    // (length, gap mask) of every skipgram in the model, by length: what the reference's matchskipgramhelper (:1722-1744) is used for — a
    // skipgram of the model can only match a window if its first word is the window's, so testing every mask of that length with has() finds the same set
    void need_reverseindex() const {
        if (this->reverseindex == NULL || this->reverseindex->empty()) {
            std::cerr << "ERROR: No reverse index present" << std::endl;
            throw InternalError();
        }
    }
    /** PatternPointer::operator==(const Pattern&) of the reference for a skipgram pointer (src/pattern.cpp:1009-1041), byte for byte */
    static bool masked_pointer_equals(const unsigned char* data, size_t bytes, uint32_t mask, const Pattern& other) {
        const size_t obytes = other.bytesize();
        auto         at     = [&](size_t i) -> unsigned char { return i < obytes ? other.data[i] : 0; };
        if (bytes == 0 || data[0] == 0) return obytes == 0;
        if (obytes == 0) return false;
        size_t tok = 0;
        for (size_t i = 0; i < bytes; ++i) {
            if (i > 0 && at(i - 1) >= 128 && at(i) == 0) return false;
            if (mask != 0 && data[i] < 128) {
                if (tok <= 30 && (mask & (1u << tok))) {
                    if (at(i) != colibri_classes::skipclass) return false;
                } else if (data[i] != at(i)) {
                    return false;
                }
                ++tok;
            } else if (data[i] != at(i)) {
                return false;
            }
        }
        return at(bytes) == colibri_classes::delimiterclass;
    }
    static void prunerelations(t_relationmap& relations, unsigned int occurrencethreshold) {  // reference :3066-3078
        for (t_relationmap::iterator it = relations.begin(); it != relations.end();) {
            if (it->second < occurrencethreshold) it = relations.erase(it);
            else ++it;
        }
    }
    /** a sentence as the relation functions see it: its tokens, and the occurrences the reverse index holds there (getreverseindex_bysentence
     *  :1849-1862) as (token, key), by position, then length, the n-gram before its skipgrams, masks ascending */
    struct RelSentence {
        std::vector<std::string>                      toks;
        std::vector<std::pair<unsigned int, Pattern>> occ;
    };
    void relation_sentence(uint32_t sentence, RelSentence& out) {
        const unsigned int sl = this->reverseindex->sentencelength((int)sentence);
        if (sl) {
            const PatternPointer whole = this->reverseindex->getpattern(IndexReference(sentence, 0), (int)sl);
            colibri_host::token_slices(whole.data, whole.bytesize(), out.toks);
        }
        for (const std::pair<IndexReference, PatternPointer>& o : this->getreverseindex_bysentence((int)sentence)) out.occ.push_back(std::make_pair((unsigned int)o.first.token, Pattern(o.second)));
    }
    /** does the occurrence of B at token i count for the occurrence of A (tokens at) at token t? (the specification: csrc/relations.hpp) */
    static bool relation_counts(int kind, const Pattern& a, const std::vector<std::string>& at, unsigned int t, unsigned int i, const Pattern& b,
                                const std::vector<std::string>& toks) {
        const unsigned int na = (unsigned int)at.size(), n = (unsigned int)b.n();
        if (kind == COLIBRI_REL_RIGHTNEIGHBOURS) return i == t + na;
        if (kind == COLIBRI_REL_LEFTNEIGHBOURS) return i + n == t;
        if (kind == COLIBRI_REL_SUBCHILDREN) {
            if (i < t || i >= t + na || n > na - (i - t)) return false;
        } else if (i > t || n < na + (t - i)) {
            return false;
        }
        auto isgap = [](const std::string& x) { return x.size() == 1 && (unsigned char)x[0] == colibri_classes::skipclass; };
        bool askip = false;
        for (const std::string& x : at) askip = askip || isgap(x);
        const bool bskip = b.category() == SKIPGRAM;
        if (b == a) {  // `candidate != pattern` (PatternPointer::operator==): a multi-byte token under a gap makes B differ from A
            bool same = true;
            for (unsigned int k = 0; k < n; ++k)
                if (isgap(at[k]) && toks[i + k].size() != 1) same = false;
            if (same) return false;
        }
        if (!askip && !bskip) return true;
        if (kind == COLIBRI_REL_SUBPARENTS) return !askip && n == na;  // A.instanceof(B): B's tokens, sliced from the corpus, are never gaps
        if (!askip || i + n > na) return false;  // Pattern(A, i, n(B)) at the corpus token index i: all of an n-gram A, or empty past the end
        bool gap = false;
        for (unsigned int k = 0; k < n; ++k) {
            if (isgap(at[i + k])) gap = true;
            else if (toks[i + k] != at[i + k]) return false;
        }
        return gap || !bskip;
    }
    t_relationmap relations_host(int kind, const Pattern& pattern, unsigned int occurrencethreshold, int category, unsigned int size, unsigned int cutoff) {
        need_reverseindex();
        IndexedData* data = this->getdata(pattern);
        if (data == NULL) throw NoSuchPattern();
        std::vector<std::string> at;
        colibri_host::token_slices(pattern.data, pattern.bytesize(), at);
        t_relationmap                  rel;
        std::map<uint32_t, RelSentence> sents;  // the sentences asked for, scanned once each
        for (const IndexReference& ref : data->data) {
            typename std::map<uint32_t, RelSentence>::iterator si = sents.find(ref.sentence);
            if (si == sents.end()) {
                si = sents.insert(std::make_pair(ref.sentence, RelSentence())).first;
                relation_sentence(ref.sentence, si->second);
            }
            const RelSentence& S = si->second;
            for (const std::pair<unsigned int, Pattern>& o : S.occ) {
                const Pattern& b = o.second;
                if (occurrencethreshold > 0 && this->occurrencecount(b) < occurrencethreshold) continue;
                if (category != 0 && (int)b.category() != category) continue;
                if (size != 0 && b.n() != size) continue;
                if (!relation_counts(kind, pattern, at, ref.token, o.first, b, S.toks)) continue;
                rel[b] += 1;
                if (cutoff > 0 && rel.size() >= cutoff) break;
            }
            if (cutoff > 0 && rel.size() >= cutoff) break;
        }
        if (occurrencethreshold > 0) prunerelations(rel, occurrencethreshold);
        return rel;
    }

  public:
    /** The skip content of a skipgram (or flexgram): for every occurrence, the tokens of the corpus from the pattern's first gap to its last
     *  gap, as a plain n-gram — the slice drops the mask (reference :3029-3059; src/pattern.cpp:853-855). Plain host code over the forward
     *  index and the loaded corpus, as in the reference: a per-pattern query, not a corpus pass. */
    t_relationmap getskipcontent(const Pattern& pattern) {
        t_relationmap skipcontent;
        if (this->reverseindex == NULL) {
            std::cerr << "ERROR: No corpus data loaded! (in PatternModel::getskipcontent)" << std::endl;
            throw InternalError();
        }
        if (pattern.category() == NGRAM) return skipcontent;
        IndexedData* data = this->getdata(pattern);
        if (data == NULL) throw NoSuchPattern();
        std::vector<std::string> toks;
        colibri_host::token_slices(pattern.data, pattern.bytesize(), toks);
        const int n = (int)toks.size();
        auto      isgap = [&](int k) { return toks[(size_t)k].size() == 1 && ((unsigned char)toks[(size_t)k][0] == colibri_classes::skipclass || (unsigned char)toks[(size_t)k][0] == colibri_classes::flexclass); };
        int       head = 0, tail = 0;  // leading / trailing tokens that are no gaps (maskheadskip / masktailskip of the reversed mask, src/algorithms.cpp:56-77)
        while (head < n && !isgap(head)) ++head;
        while (tail < n - head && !isgap(n - tail - 1)) ++tail;
        for (const IndexReference& ref : data->data) {
            const PatternPointer     raw = this->reverseindex->getpattern(ref, n);
            std::vector<std::string> w;
            colibri_host::token_slices(raw.data, raw.bytesize(), w);
            std::string content;
            for (int k = head; k < n - tail; ++k) content += w[(size_t)k];
            skipcontent[Pattern((const unsigned char*)content.data(), content.size())] += 1;
        }
        return skipcontent;
    }
    /** the n-grams of the model that instantiate the given skipgram / flexgram at its occurrences (reference :3127-3165 over getreverseindex
     *  :1746-1824 with category NGRAM: the window of the pattern's own length at each occurrence, if the model has it) */
    t_relationmap getinstances(const Pattern& pattern, unsigned int occurrencethreshold = 0) {
        need_reverseindex();
        IndexedData* data = this->getdata(pattern);
        if (data == NULL) throw NoSuchPattern();
        t_relationmap instances;
        const int     n = (int)pattern.n();
        if (n >= this->minlength() && n <= this->maxlength()) {
            for (const IndexReference& ref : data->data) {
                if (ref.token + (unsigned int)n > this->reverseindex->sentencelength((int)ref.sentence)) continue;
                const Pattern candidate(this->reverseindex->getpattern(ref, n));
                if (candidate.category() != NGRAM || candidate == pattern) continue;
                if (occurrencethreshold == 0 ? !this->has(candidate) : this->occurrencecount(candidate) < occurrencethreshold) continue;
                instances[candidate] += 1;
            }
        }
        if (occurrencethreshold > 0) prunerelations(instances, occurrencethreshold);
        return instances;
    }
    /** the skipgrams of the model that abstract over the given pattern at its occurrences (reference :3086-3118): every gap mask a skipgram
     *  of this length has in the model, laid over the window at each occurrence */
    t_relationmap gettemplates(const Pattern& pattern, unsigned int occurrencethreshold = 0) {
        need_reverseindex();
        IndexedData* data = this->getdata(pattern);
        if (data == NULL) throw NoSuchPattern();
        t_relationmap templates;
        const int     n = (int)pattern.n();
        if (this->hasskipgrams() && n >= 3 && n >= this->minlength() && n <= this->maxlength() &&
            (occurrencethreshold == 0 || this->occurrencecount(pattern) >= occurrencethreshold)) {
            this->compute_skipmasks();
            const std::vector<uint32_t>& masks = this->skipmasks_[n];
            for (const IndexReference& ref : data->data) {
                if (ref.token + (unsigned int)n > this->reverseindex->sentencelength((int)ref.sentence)) continue;
                PatternPointer window = this->reverseindex->getpattern(ref, n);
                for (uint32_t mask : masks) {
                    window.mask = mask;
                    const Pattern candidate(window);
                    if (candidate.category() != SKIPGRAM || !this->has(candidate)) continue;
                    // The reference drops the pattern itself with `candidate != pattern`: a masked pointer into the corpus against the
                    // materialised pattern, compared byte by byte AT THE SAME INDEX (src/pattern.cpp:1009-1041). That recognises the pattern only
                    // where every token under a gap is a single byte (elsewhere a skipgram is listed as its own template), and it takes an
                    // n-gram for the candidate when the low byte of the token under the gap happens to be 03 — reproduced, not corrected.
                    if (masked_pointer_equals(window.data, (size_t)window.bytesize(), mask, pattern)) continue;
                    templates[candidate] += 1;
                }
            }
        }
        if (occurrencethreshold > 0) prunerelations(templates, occurrencethreshold);
        return templates;
    }
    /** the four relation kinds the device computes for the whole model (COLIBRI_REL_*), by filter name (reference :3622-3662, labels swapped
     *  against the functions there); -1 for any other filter */
    static int relation_kind(const std::string& filter, std::string* label = NULL) {
        int         k = -1;
        const char* l = "";
        if (filter == "subparents" || filter == "subsumed") k = COLIBRI_REL_SUBPARENTS, l = "SUBSUMED-BY";
        else if (filter == "subchildren" || filter == "subsumes") k = COLIBRI_REL_SUBCHILDREN, l = "SUBSUMES";
        else if (filter == "rightneighbours" || filter == "rightneighbors") k = COLIBRI_REL_LEFTNEIGHBOURS, l = "RIGHT-NEIGHBOUR-OF";
        else if (filter == "leftneighbours" || filter == "leftneighbors") k = COLIBRI_REL_RIGHTNEIGHBOURS, l = "LEFT-NEIGHBOUR-OF";
        if (label) *label = l;
        return k;
    }
    /** getsubchildren / getsubparents / getleftneighbours / getrightneighbours of one pattern (reference :3166-3352; the specification is in
     *  include/colibri_hip.h and csrc/relations.hpp). Plain host code over the forward index and the loaded corpus, a per-pattern query: the CLI's
     *  relation loop (outputrelations_model) runs the whole model on the device. cutoff: the neighbours stop at that many distinct patterns, in the
     *  order this scan meets them — the forward index, then by position, length, the n-gram before its skipgrams, masks ascending (the
     *  reference's order is its unordered_set's) */
    t_relationmap getsubchildren(const Pattern& pattern, unsigned int occurrencethreshold = 0, int category = 0, unsigned int size = 0) {
        return relations_host(COLIBRI_REL_SUBCHILDREN, pattern, occurrencethreshold, category, size, 0);
    }
    t_relationmap getsubparents(const Pattern& pattern, unsigned int occurrencethreshold = 0, int category = 0, unsigned int size = 0) {
        return relations_host(COLIBRI_REL_SUBPARENTS, pattern, occurrencethreshold, category, size, 0);
    }
    t_relationmap getleftneighbours(const Pattern& pattern, unsigned int occurrencethreshold = 0, int category = 0, unsigned int size = 0, unsigned int cutoff = 0) {
        return relations_host(COLIBRI_REL_LEFTNEIGHBOURS, pattern, occurrencethreshold, category, size, cutoff);
    }
    t_relationmap getrightneighbours(const Pattern& pattern, unsigned int occurrencethreshold = 0, int category = 0, unsigned int size = 0, unsigned int cutoff = 0) {
        return relations_host(COLIBRI_REL_RIGHTNEIGHBOURS, pattern, occurrencethreshold, category, size, cutoff);
    }
    /** one relation of every pattern of the model on the device (the four functions above with category 0, size 0, no cutoff, or getinstances /
     *  gettemplates as COLIBRI_REL_INSTANCES / COLIBRI_REL_TEMPLATES): `keys` receives
     *  the model's patterns in the numbering of the rows. After a --gpus N build the rows come from the model uploaded to one device */
    void computerelations_device(int kind, unsigned int threshold, colibri_host::RelationRows& rows, std::vector<Pattern>& keys) {
        need_reverseindex();
        keys.clear();
        if (this->result && this->result->device && colibri_host::device_relations_resident(this->result->device, *this->result, kind, threshold, rows)) {
            const colibri_host::TrainResult& r = *this->result;
            for (size_t j = 0; j < r.size(); ++j) keys.push_back(Pattern(r.key_bytes.data() + r.key_off[j], (size_t)(r.key_off[j + 1] - r.key_off[j])));
            return;
        }
        std::vector<uint64_t>      key_off(1, 0), ref_off(1, 0);
        std::vector<unsigned char> key_bytes;
        std::vector<uint32_t>      rs;
        std::vector<uint16_t>      rt;
        for (typename MapType::iterator it = this->begin(); it != this->end(); ++it) {
            key_bytes.insert(key_bytes.end(), it->first.data, it->first.data + it->first.bytesize());
            key_off.push_back(key_bytes.size());
            for (const IndexReference& ref : it->second.data) {
                rs.push_back(ref.sentence);
                rt.push_back(ref.token);
            }
            ref_off.push_back(rs.size());
            keys.push_back(it->first);
        }
        colibri_host::device_relations(key_off, key_bytes.data(), ref_off, rs.data(), rt.data(), this->reverseindex->beginpointer(), this->reverseindex->bytesize(), kind, threshold,
                                       rows);
    }
    /** getskipcontent of every pattern of the model on the device (one call; csrc/skiprel.hpp): `keys` receives the model's patterns in the numbering
     *  of the rows, `contents` the content of each row as a pattern. rows.b = the content's number in `keys`, or 0xFFFFFFFF when the model does not
     *  hold it. A reference whose window leaves its sentence is skipped (a trained model has none). After a --gpus N build the rows come from the
     *  model uploaded to one device */
    void computeskipcontent_device(colibri_host::SkipContentRows& rows, std::vector<Pattern>& keys, std::vector<Pattern>& contents) {
        need_reverseindex();
        keys.clear();
        contents.clear();
        if (this->result && this->result->device && colibri_host::device_skipcontent_resident(this->result->device, *this->result, rows)) {
            const colibri_host::TrainResult& r = *this->result;
            for (size_t j = 0; j < r.size(); ++j) keys.push_back(Pattern(r.key_bytes.data() + r.key_off[j], (size_t)(r.key_off[j + 1] - r.key_off[j])));
        } else {
            std::vector<uint64_t>      key_off(1, 0), ref_off(1, 0);
            std::vector<unsigned char> key_bytes;
            std::vector<uint32_t>      rs;
            std::vector<uint16_t>      rt;
            for (typename MapType::iterator it = this->begin(); it != this->end(); ++it) {
                key_bytes.insert(key_bytes.end(), it->first.data, it->first.data + it->first.bytesize());
                key_off.push_back(key_bytes.size());
                for (const IndexReference& ref : it->second.data) {
                    rs.push_back(ref.sentence);
                    rt.push_back(ref.token);
                }
                ref_off.push_back(rs.size());
                keys.push_back(it->first);
            }
            colibri_host::device_skipcontent(key_off, key_bytes.data(), ref_off, rs.data(), rt.data(), this->reverseindex->beginpointer(), this->reverseindex->bytesize(), rows);
        }
        for (size_t i = 0; i < rows.a.size(); ++i)
            contents.push_back(Pattern(rows.content_bytes.data() + rows.content_off[i], (size_t)(rows.content_off[i + 1] - rows.content_off[i])));
    }
    /** the rows of one device call printed as outputrelations prints them: every pattern of the model, the header before the first one's rows, then
     *  its rows (a = the row's pattern number in `keys`) in the order given. rhs(r) is row r's right-hand side, count2(r) its COUNT2 */
    template <class Rhs, class Count2>
    void outputrows_device(const ClassDecoder& classdecoder, std::ostream& OUT, const std::string& label, const std::vector<Pattern>& keys, const std::vector<uint32_t>& a,
                           const std::vector<uint32_t>& count, Rhs rhs, Count2 count2) {
        t_relationmap number;  // pattern -> its number in `keys`
        for (size_t j = 0; j < keys.size(); ++j) number[keys[j]] = (uint32_t)j;
        std::vector<uint64_t> first_row(keys.size() + 1, 0);  // rows of pattern j: [first_row[j], first_row[j + 1])
        for (size_t i = 0; i < a.size(); ++i) ++first_row[a[i] + 1];
        for (size_t j = 0; j < keys.size(); ++j) first_row[j + 1] += first_row[j];
        bool first = true;
        for (typename MapType::iterator it = this->begin(); it != this->end(); ++it) {
            OUT << it->first.tostring(classdecoder) << std::endl;
            if (first) OUT << "#\tPATTERN1\tRELATION\tPATTERN2\tREL.COUNT\tREL.FREQUENCY\tCOUNT2" << std::endl;
            first = false;
            t_relationmap::iterator at = number.find(it->first);
            if (at == number.end()) continue;
            const uint64_t r0 = first_row[at->second], r1 = first_row[at->second + 1];
            int            total = 0;
            for (uint64_t r = r0; r < r1; ++r) total += (int)count[r];
            if (total == 0) continue;
            const double      total_f   = total;
            const std::string pattern_s = it->first.tostring(classdecoder);
            for (uint64_t r = r0; r < r1; ++r)
                OUT << "\t" << pattern_s << "\t" << label << "\t" << rhs(r).tostring(classdecoder) << "\t" << count[r] << "\t" << count[r] / total_f << "\t" << count2(r) << std::endl;
        }
    }
    /** the CLI's relation loop for --subsumes / --subsumed / --leftneighbours / --rightneighbours: the rows of every pattern from one device call,
     *  printed as outputrelations prints them (header before the first pattern; within a pattern by count descending, then B's key bytes).
     *  --skipcontent takes the same way under COLIBRI_SKIPREL=device (COUNT2 = the content's own count in the model, or 0); unset, `auto` or
     *  `host` keep the per-pattern host loop (no break-even is measured) */
    void outputrelations_model(const ClassDecoder& classdecoder, std::ostream& OUT, const std::string& filter) override {
        std::string label;
        const int   kind = relation_kind(filter, &label);
        if (kind < 0) {
            const char* where = std::getenv("COLIBRI_SKIPREL");
            if (filter == "skipcontent" && where && std::string(where) == "device") {
                colibri_host::SkipContentRows rows;
                std::vector<Pattern>          keys, contents;
                computeskipcontent_device(rows, keys, contents);
                outputrows_device(classdecoder, OUT, "INSTANTIATED-BY", keys, rows.a, rows.count, [&](uint64_t r) -> const Pattern& { return contents[r]; },
                                  [&](uint64_t r) { return rows.b[r] == 0xFFFFFFFFu ? 0u : (unsigned int)this->occurrencecount(keys[rows.b[r]]); });
                return;
            }
            bool first = true;
            for (typename MapType::iterator it = this->begin(); it != this->end(); ++it) {
                OUT << it->first.tostring(classdecoder) << std::endl;
                this->outputrelations(it->first, classdecoder, OUT, filter, first);
                first = false;
            }
            return;
        }
        colibri_host::RelationRows rows;
        std::vector<Pattern>       keys;
        computerelations_device(kind, 0u, rows, keys);
        outputrows_device(classdecoder, OUT, label, keys, rows.a, rows.count, [&](uint64_t r) -> const Pattern& { return keys[rows.b[r]]; },
                          [&](uint64_t r) { return this->occurrencecount(keys[rows.b[r]]); });
    }
    /** one row per related pattern (reference :3595-3609) */
    void outputrelations(const Pattern& pattern, t_relationmap& relations, const ClassDecoder& classdecoder, std::ostream& OUT, const std::string& label = "RELATED-TO") {
        int total = 0;
        for (t_relationmap::iterator it = relations.begin(); it != relations.end(); ++it) total += (int)it->second;
        if (total == 0) return;
        const double      total_f   = total;
        const std::string pattern_s = pattern.tostring(classdecoder);
        for (t_relationmap::iterator it = relations.begin(); it != relations.end(); ++it)
            OUT << "\t" << pattern_s << "\t" << label << "\t" << it->first.tostring(classdecoder) << "\t" << it->second << "\t" << it->second / total_f << "\t"
                << this->occurrencecount(it->first) << std::endl;
    }
    /** the relations of a pattern selected by `filter` (reference :3622-3662). Built here: skipcontent. "instances" and "templates" print
     *  nothing through this entry point in the reference either — its call with a PatternPointer resolves to the base class's empty
     *  getinstances / gettemplates(const PatternPointer&) (:2635-2640), the working ones take a Pattern (used directly, src/test.cpp:1457) */
    void outputrelations(const Pattern& pattern, const ClassDecoder& classdecoder, std::ostream& OUT, const std::string& filter = "", bool outputheader = true) override {
        std::string label;
        const int   kind = relation_kind(filter, &label);
        if (kind >= 0) {
            if (outputheader) OUT << "#\tPATTERN1\tRELATION\tPATTERN2\tREL.COUNT\tREL.FREQUENCY\tCOUNT2" << std::endl;
            t_relationmap relations = relations_host(kind, pattern, 0, 0, 0, 0);
            this->outputrelations(pattern, relations, classdecoder, OUT, label);
            return;
        }
        if (filter != "skipcontent" && filter != "instances" && filter != "templates") {
            std::cerr << "ERROR: relation '" << (filter.empty() ? "all" : filter) << "' is not part of the MI355X-accelerated build (see DESIGN.md, out of scope)" << std::endl;
            throw InternalError();
        }
        if (outputheader) OUT << "#\tPATTERN1\tRELATION\tPATTERN2\tREL.COUNT\tREL.FREQUENCY\tCOUNT2" << std::endl;
        if (filter == "skipcontent") {
            t_relationmap relations = this->getskipcontent(pattern);
            this->outputrelations(pattern, relations, classdecoder, OUT, "INSTANTIATED-BY");
        }
    }
    /** The patterns of the model that co-occur with `pattern` in a sentence (reference :3542-3576): for every reference of the pattern in its
     *  forward index, every occurrence the corpus scan finds in that sentence (getreverseindex :1746-1824: every window of minlength()..maxlength()
     *  tokens the model has, and for n >= 3 that window under each gap mask of the model's skipgrams of length n) counts when it lies wholly
     *  before or after the pattern with at least one token between them; the pattern itself counts too. occurrencethreshold > 0: the neighbour's
     *  own count must reach it, and so must the joint count. Plain host code over the forward index and the loaded corpus, a per-pattern query:
     *  computecooc / outputcooc run the whole model on the device. */
    t_relationmap getcooc(const Pattern& pattern, unsigned int occurrencethreshold = 0) {
        need_reverseindex();
        IndexedData* data = this->getdata(pattern);
        if (data == NULL) throw NoSuchPattern();
        const unsigned int na = (unsigned int)pattern.n();
        t_relationmap      cooc;
        std::map<uint32_t, std::vector<std::pair<unsigned int, Pattern>>> rev;  // the reverse index of the sentences asked for, built once each
        for (const IndexReference& ref : data->data) {
            std::vector<std::pair<unsigned int, Pattern>>& occ = rev[ref.sentence];
            if (occ.empty()) {
                for (const std::pair<IndexReference, PatternPointer>& o : this->getreverseindex_bysentence((int)ref.sentence)) occ.push_back(std::make_pair((unsigned int)o.first.token, Pattern(o.second)));
                if (occ.empty()) occ.push_back(std::make_pair(~0u, Pattern()));  // (an empty sentence: remembered as looked at)
            }
            for (const std::pair<unsigned int, Pattern>& o : occ) {
                if (o.first == ~0u) continue;
                const unsigned int n2 = (unsigned int)o.second.n();
                if (!(o.first + n2 < ref.token || o.first > ref.token + na)) continue;
                if (occurrencethreshold > 0 && this->occurrencecount(o.second) < occurrencethreshold) continue;
                cooc[o.second] += 1;
            }
        }
        if (occurrencethreshold > 0) prunerelations(cooc, occurrencethreshold);
        return cooc;
    }
    /** normalised pointwise mutual information of two patterns and their joint count (reference :3582-3587; the counts are size_t there, so their
     *  product does not wrap; the group total is an unsigned int) */
    double npmi(const Pattern& key1, const Pattern& key2, int jointcount) {
        return log((double)jointcount / ((size_t)this->occurrencecount(key1) * (size_t)this->occurrencecount(key2))) /
               -log((double)jointcount / (double)this->totaloccurrencesingroup(0, 0));
    }
    /** the co-occurrence table of the whole model on the device (getcooc over every pattern, reference :3700-3719 / :3671-3691): `keys` receives the
     *  model's patterns in the numbering of the rows. mode COLIBRI_COOC_COUNT keeps joint counts >= threshold, COLIBRI_COOC_NPMI values >= x */
    void computecooc_device(int mode, unsigned int threshold, double x, colibri_host::CoocRows& rows, std::vector<Pattern>& keys) {
        need_reverseindex();
        keys.clear();
        if (this->result && this->result->device && colibri_host::device_cooc_resident(this->result->device, *this->result, threshold, mode, x, rows)) {
            const colibri_host::TrainResult& r = *this->result;
            for (size_t j = 0; j < r.size(); ++j) keys.push_back(Pattern(r.key_bytes.data() + r.key_off[j], (size_t)(r.key_off[j + 1] - r.key_off[j])));
            return;
        }
        std::vector<uint64_t>      key_off(1, 0), ref_off(1, 0);
        std::vector<unsigned char> key_bytes;
        std::vector<uint32_t>      rs;
        std::vector<uint16_t>      rt;
        for (typename MapType::iterator it = this->begin(); it != this->end(); ++it) {
            key_bytes.insert(key_bytes.end(), it->first.data, it->first.data + it->first.bytesize());
            key_off.push_back(key_bytes.size());
            for (const IndexReference& ref : it->second.data) {
                rs.push_back(ref.sentence);
                rt.push_back(ref.token);
            }
            ref_off.push_back(rs.size());
            keys.push_back(it->first);
        }
        colibri_host::device_cooc(key_off, key_bytes.data(), ref_off, rs.data(), rt.data(), this->reverseindex->beginpointer(), this->reverseindex->bytesize(), threshold, mode, x, rows);
    }
    /** the reference's whole-model entry points (:3700-3719, :3671-3691, both directions): coocmap[A][B] = joint count >= threshold / NPMI >= threshold,
     *  computed on the device */
    void computecooc(std::map<Pattern, t_relationmap>& coocmap, int threshold) {
        colibri_host::CoocRows rows;
        std::vector<Pattern>   keys;
        computecooc_device(COLIBRI_COOC_COUNT, threshold > 0 ? (unsigned int)threshold : 0u, 0.0, rows, keys);
        for (size_t i = 0; i < rows.a.size(); ++i) coocmap[keys[rows.a[i]]][keys[rows.b[i]]] = rows.count[i];
    }
    void computenpmi(std::map<Pattern, t_relationmap_double>& coocmap, double threshold) {
        colibri_host::CoocRows rows;
        std::vector<Pattern>   keys;
        computecooc_device(COLIBRI_COOC_NPMI, 0u, threshold, rows, keys);
        for (size_t i = 0; i < rows.a.size(); ++i) coocmap[keys[rows.a[i]]][keys[rows.b[i]]] = rows.value[i];
    }
    /** -C: the header and one row per (pattern, co-occurring pattern) with a joint count >= threshold, ordered by count descending, then by the two
     *  patterns' key bytes (reference :3808-3829; the threshold arrives as a double and is used as an int, :3712). The reference's own order of
     *  equal counts is not reproducible, and its loop reads freed memory */
    void outputcooc(std::ostream& OUT, const ClassDecoder& classdecoder, double threshold) override {
        std::cerr << "Collecting patterns and computing co-occurrence..." << std::endl;
        colibri_host::CoocRows rows;
        std::vector<Pattern>   keys;
        const int              t = (int)threshold;
        computecooc_device(COLIBRI_COOC_COUNT, t > 0 ? (unsigned int)t : 0u, 0.0, rows, keys);
        std::cerr << "Building inverse map..." << std::endl;
        OUT << "Pattern1\tPattern2\tCooc" << std::endl;
        for (size_t i = 0; i < rows.a.size(); ++i)
            OUT << keys[rows.a[i]].tostring(classdecoder) << "\t" << keys[rows.b[i]].tostring(classdecoder) << "\t" << rows.count[i] << std::endl;
    }
    /** -Y: the same with normalised PMI values >= threshold (reference :3780-3804) */
    void outputcooc_npmi(std::ostream& OUT, const ClassDecoder& classdecoder, double threshold) override {
        std::cerr << "Collecting patterns and computing NPMI..." << std::endl;
        colibri_host::CoocRows rows;
        std::vector<Pattern>   keys;
        computecooc_device(COLIBRI_COOC_NPMI, 0u, threshold, rows, keys);
        std::cerr << "Building inverse map..." << std::endl;
        OUT << "Pattern1\tPattern2\tNPMI" << std::endl;
        for (size_t i = 0; i < rows.a.size(); ++i)
            OUT << keys[rows.a[i]].tostring(classdecoder) << "\t" << keys[rows.b[i]].tostring(classdecoder) << "\t" << rows.value[i] << std::endl;
    }
    /** Compute flexgrams by abstracting from the skipgrams in the model (reference :3724-3744): every skipgram's references are appended to
     *  the flexgram it abstracts to (Pattern::toflexgram). The group-by and the merge of the reference lists run on the device
     *  (colibri_flexgrams); each flexgram's new references arrive ascending. @return the number of flexgrams that were not in the model */
    int computeflexgrams_fromskipgrams() override {
        colibri_host::TrainResult flex;
        if (this->result && this->result->device) {  // the model is still in HBM: group and merge there, only the flexgrams come back
            colibri_host::device_flexgrams_resident(this->result->device, flex);
            this->result->device.reset();
        } else if (this->result) {  // device results not materialised yet: their flat arrays are the input
            std::shared_ptr<colibri_host::TrainResult> r = this->result;
            colibri_host::device_flexgrams(r->key_off, r->key_bytes.data(), r->ref_off, r->ref_sentence.data(), r->ref_token.data(), flex);
        } else {
            std::vector<uint64_t>      key_off(1, 0), ref_off(1, 0);
            std::vector<unsigned char> key_bytes;
            std::vector<uint32_t>      rs;
            std::vector<uint16_t>      rt;
            for (typename MapType::iterator it = this->begin(); it != this->end(); ++it) {
                if (it->first.category() != SKIPGRAM) continue;
                key_bytes.insert(key_bytes.end(), it->first.data, it->first.data + it->first.bytesize());
                key_off.push_back(key_bytes.size());
                for (const IndexReference& ref : it->second.data) {
                    rs.push_back(ref.sentence);
                    rt.push_back(ref.token);
                }
                ref_off.push_back(rs.size());
            }
            rs.push_back(0);
            rt.push_back(0);
            colibri_host::device_flexgrams(key_off, key_bytes.data(), ref_off, rs.data(), rt.data(), flex);
        }
        if (this->result) {
            // the model has not been turned into map nodes yet: the flexgrams are appended to its flat arrays (no pattern of a freshly trained model
            // is a flexgram — a corpus with a literal {**} token is refused at upload — so every one of them is new)
            colibri_host::TrainResult& r   = *this->result;
            this->flatindex.reset();  // (built over the arrays as they were)
            r.device_current = false;
            const size_t               np  = r.size(), nf = flex.size();
            const uint64_t             kb  = r.key_off[np], nr = r.ref_off[np], fkb = flex.key_off[nf], fnr = flex.ref_off[nf];
            r.key_bytes.resize((size_t)(kb + fkb) + 1);
            std::memcpy(r.key_bytes.data() + kb, flex.key_bytes.data(), (size_t)fkb);
            r.ref_sentence.resize((size_t)(nr + fnr) + 1);
            r.ref_token.resize((size_t)(nr + fnr) + 1);
            std::memcpy(r.ref_sentence.data() + nr, flex.ref_sentence.data(), (size_t)fnr * sizeof(uint32_t));
            std::memcpy(r.ref_token.data() + nr, flex.ref_token.data(), (size_t)fnr * sizeof(uint16_t));
            r.key_off.resize(np + nf + 1);
            r.ref_off.resize(np + nf + 1);
            r.counts.resize(np + nf);
            for (size_t j = 0; j < nf; ++j) {
                r.key_off[np + j + 1] = kb + flex.key_off[j + 1];
                r.ref_off[np + j + 1] = nr + flex.ref_off[j + 1];
                r.counts[np + j]      = flex.counts[j];
            }
            r.stats.npatterns = np + nf;
            return (int)nf;
        }
        int count = 0;
        for (size_t j = 0; j < flex.size(); ++j) {
            const Pattern flexgram(flex.key_bytes.data() + flex.key_off[j], (size_t)(flex.key_off[j + 1] - flex.key_off[j]));
            if (!this->has(flexgram)) ++count;
            IndexedData& d = (*this)[flexgram];
            d.data.reserve(d.data.size() + (size_t)(flex.ref_off[j + 1] - flex.ref_off[j]));
            for (uint64_t k = flex.ref_off[j]; k < flex.ref_off[j + 1]; ++k) d.data.push_back(IndexReference(flex.ref_sentence[k], flex.ref_token[k]));
        }
        return count;
    }
    /** Train skipgrams on a model that holds its n-grams (reference :2969-3010; what colibri-patternmodeller -i model -s runs, and the way one n-gram
     *  count is reused under other -t / -T / -l): for n = 3 .. MAXLENGTH every n-gram of n tokens whose two (n-1)-token parts are still in the model
     *  (MINTOKENS or MINTOKENS_SKIPGRAMS above 1) hands its references to its skipgram under every gap mask; an order that finds none ends the loop
     *  unpruned, otherwise every pattern of n tokens below MINTOKENS goes — n-grams too — and then every skipgram with fewer than MINSKIPTYPES source
     *  n-grams. All of it runs on the device (colibri_modelskip), on the model where a train() left it in HBM, on the flat arrays of a run
     *  not yet turned into map nodes, or on arrays gathered from the map; no corpus is needed, and every new list arrives ascending. constrainbymodel
     *  == this is trainskipgrams_selfconstrained, as in the reference; any other constraint is refused, as is a model that holds skipgrams or flexgrams
     *  already (their references would be added a second time) or an indexed model without a single reference. */
    void trainskipgrams(const PatternModelOptions& in_options, PatternModelInterface* constrainbymodel = NULL) {
        PatternModelOptions options = in_options;
        if (options.MINTOKENS == -1) options.MINTOKENS = 2;
        if (constrainbymodel == this) {
            this->trainskipgrams_selfconstrained(options);
            return;
        }
        if (constrainbymodel != NULL) {
            std::cerr << "ERROR: trainskipgrams constrained by another model is not on the MI355X-accelerated path (NULL or the model itself are)" << std::endl;
            throw InternalError();
        }
        colibri_options o{};
        o.mintokens           = options.MINTOKENS;
        o.mintokens_skipgrams = options.MINTOKENS_SKIPGRAMS;
        o.minskiptypes        = options.MINSKIPTYPES;
        o.maxlength           = options.MAXLENGTH;
        o.maxskips            = options.MAXSKIPS;
        colibri_host::SkipgramAnswer answer;
        colibri_host::SkipgramLog    log;
        std::vector<Pattern>         order;  // the map's patterns in the order of the gathered arrays
        const char*                  form = "resident";
        auto refuse_empty = [](uint64_t np, uint64_t nrefs) {
            if (np == 0 || nrefs != 0) return;
            std::cerr << "ERROR: trainskipgrams needs the model's forward index, and this indexed model holds no reference (an unindexed model file read as indexed?)" << std::endl;
            throw InternalError();
        };
        if (this->result) {  // (a run that was asked for skipgrams and found some is refused by the device call: its keys hold the gap byte)
            colibri_host::TrainResult& r = *this->result;
            refuse_empty(r.size(), r.size() ? r.ref_off[r.size()] : 0);
            if (!(r.device && colibri_host::device_modelskip_resident(r.device, r, o, answer, log))) {  // device results not materialised yet: their flat arrays are the input
                form = "uploaded";
                colibri_host::device_modelskip(r.key_off, r.key_bytes.data(), r.ref_off, r.ref_sentence.data(), r.ref_token.data(), o, answer, log);
            }
        } else {
            form = "uploaded";
            std::vector<uint64_t>      key_off(1, 0), ref_off(1, 0);
            std::vector<unsigned char> key_bytes;
            std::vector<uint32_t>      rs;
            std::vector<uint16_t>      rt;
            order.reserve(this->size());
            for (typename MapType::iterator it = this->begin(); it != this->end(); ++it) {
                if (it->first.category() != NGRAM) {
                    std::cerr << "ERROR: the model holds skipgrams or flexgrams already: trainskipgrams would add every reference a second time (load the n-grams only, or "
                                 "rebuild in place with -I -s)" << std::endl;
                    throw InternalError();
                }
                key_bytes.insert(key_bytes.end(), it->first.data, it->first.data + it->first.bytesize());
                key_off.push_back(key_bytes.size());
                for (const IndexReference& ref : it->second.data) {
                    rs.push_back(ref.sentence);
                    rt.push_back(ref.token);
                }
                ref_off.push_back(rs.size());
                order.push_back(it->first);
            }
            refuse_empty(order.size(), rs.size());
            rs.push_back(0);
            rt.push_back(0);
            colibri_host::device_modelskip(key_off, key_bytes.data(), ref_off, rs.data(), rt.data(), o, answer, log);
        }
        const size_t np = this->result ? this->result->size() : order.size();
        if (colibri_host::skipgram_answer_fault(answer, np) != NULL) {  // (before anything changes)
            std::cerr << "ERROR: colibri_modelskip's answer is malformed: " << colibri_host::skipgram_answer_fault(answer, np) << std::endl;
            throw InternalError();
        }
        // the reference's progress lines, from the per-order figures (`total kept` in its unsigned 32-bit arithmetic, n-grams among the pruned)
        if (!options.QUIET) std::cerr << "Finding skipgrams on the basis of extracted n-grams..." << std::endl;
        if (std::getenv("COLIBRI_HOST_TIMING") != NULL) std::cerr << "(skipgrams of the loaded model on the device: " << form << " model)" << std::endl;
        bool found_any = false;
        for (uint32_t i = 0; i < log.orders; ++i) {
            const int n = 3 + (int)i;
            if (!options.QUIET) std::cerr << "Counting " << n << "-skipgrams" << std::endl;
            const unsigned int found = (unsigned int)log.found[n], pruned = (unsigned int)log.pruned[n], extra = (unsigned int)log.extra[n];
            if (!found) {
                std::cerr << " None found" << std::endl;
                break;
            }
            found_any = true;
            if (options.QUIET) continue;
            std::cerr << " Found " << found << " skipgrams...pruned " << pruned;
            if (extra) std::cerr << " plus " << extra << " extra skipgrams..";
            std::cerr << "...total kept: " << found - pruned - extra << std::endl;
        }
        if (colibri_host::skipgram_answer_changes_nothing(answer)) {  // (no skipgram kept, no pattern erased: the model, its look-up table and its resident copy stay)
            if (found_any) this->hasskipgrams_ = true;
            return;
        }
        if (this->result) {
            colibri_host::TrainResult& r = *this->result;
            if (!colibri_host::skipgram_merge_flat(r.key_off, r.key_bytes, r.counts, r.ref_off, r.ref_sentence, r.ref_token, answer)) {  // (refused whole: nothing was touched)
                std::cerr << "ERROR: trainskipgrams: the run's arrays are not a model in export layout, the skipgrams were not installed" << std::endl;
                throw InternalError();
            }
            this->flatindex.reset();  // (built over the arrays as they were)
            r.device_current  = false;
            r.stats.npatterns = r.size();
        } else {
            colibri_host::skipgram_merge_each(  // (the answer was checked above: it is not refused here)
                answer, order.size(), [&](size_t j) { this->erase(order[j]); },
                [&](const unsigned char* key, size_t len, const uint32_t* s, const uint16_t* t, size_t nrefs) {
                    IndexedData& d = (*this)[Pattern(key, len)];
                    d.data.reserve(d.data.size() + nrefs);
                    for (size_t k = 0; k < nrefs; ++k) d.data.push_back(IndexReference(s[k], t[k]));
                });
        }
        if (found_any) this->hasskipgrams_ = true;
        this->cache_grouptotal.clear();  // (forces recomputation of the statistics, as the reference does)
        this->cache_grouptotalpatterns.clear();
        this->cache_grouptotalwordtypes.clear();
        this->cache_grouptotaltokens.clear();
        this->skipmasks_size_ = (size_t)-1;
    }
    void train(std::istream* in, const PatternModelOptions& options, PatternModelInterface* constrainbymodel = NULL, PatternSet<>* filter = NULL, bool continued = false,
               uint32_t firstsentence = 1, bool ignoreerrors = false) override {
        if (options.DOSKIPGRAMS && this->reverseindex == NULL) {  // reference :2828-2833
            std::cerr << "ERROR: You must specify a reverse index if you want to train skipgrams (or train skipgrams exhaustively)" << std::endl;
            throw InternalError();
        }
        PatternModel<IndexedData, IndexedDataHandler, MapType>::train(in, options, constrainbymodel, filter, continued, firstsentence, ignoreerrors);
    }
    void train(const std::string& filename, const PatternModelOptions& options, PatternModelInterface* constrainbymodel = NULL, PatternSet<>* filter = NULL, bool continued = false,
               uint32_t firstsentence = 1, bool ignoreerrors = false) override {
        if (options.DOSKIPGRAMS && this->reverseindex == NULL) {
            std::cerr << "ERROR: You must specify a reverse index if you want to train skipgrams (or train skipgrams exhaustively)" << std::endl;
            throw InternalError();
        }
        PatternModel<IndexedData, IndexedDataHandler, MapType>::train(filename, options, constrainbymodel, filter, continued, firstsentence, ignoreerrors);
    }
};

// ---- model comparison (reference src/patternmodel.cpp:22-171; the C ABI's colibri_compare) --------------------------------------------------------

/** log-likelihood of one pattern across the models (reference :22-63): host code, the reference's expression and order of evaluation */
inline double comparemodels_loglikelihood(const Pattern pattern, const std::vector<PatternModel<uint32_t>*>& models) {
    if (models.size() < 2) {
        std::cerr << "compare_models_loglikelihood requires at least two models!" << std::endl;
        throw InternalError();
    }
    unsigned long long  n_sum = 0, o_sum = 0;
    std::vector<int>    observed, total;
    std::vector<double> expected;
    for (const auto& model : models) {
        const int o = (int)model->occurrencecount(pattern);
        const int n = (int)model->tokens();
        total.push_back(n);
        n_sum += n;
        observed.push_back(o);
        o_sum += o;
    }
    for (size_t i = 0; i < total.size(); i++) expected.push_back(exp((log(total[i]) + log(o_sum)) - log(n_sum)));
    double ll = 0;
    for (size_t i = 0; i < models.size(); i++)
        if (observed[i] > 0) ll += observed[i] * log(observed[i] / expected[i]);
    ll = ll * 2;
    if (std::isnan(ll)) ll = 0;
    return ll;
}

namespace colibri_host {
/** the models' keys and counts in export layout, then one device_compare call */
struct CompareBatch {
    std::vector<std::vector<uint64_t>>      off;
    std::vector<std::vector<unsigned char>> bytes;
    std::vector<std::vector<uint32_t>>      counts;
    CompareRows                             rows;
    void run(std::vector<PatternModel<uint32_t>*>& models, bool conjunctiononly, bool sorted) {
        if (models.size() < 2) {
            std::cerr << "compare_models_loglikelihood requires at least two models!" << std::endl;
            throw InternalError();
        }
        const size_t N = models.size();
        off.resize(N);
        bytes.resize(N);
        counts.resize(N);
        std::vector<CompareInput> in(N);
        for (size_t m = 0; m < N; ++m) {
            models[m]->collect_counts(off[m], bytes[m], counts[m]);
            in[m].key_off   = off[m].data();
            in[m].key_bytes = bytes[m].data();
            in[m].counts    = counts[m].data();
            in[m].npatterns = off[m].size() - 1;
            in[m].tokens    = models[m]->tokens();
        }
        device_compare(in, conjunctiononly, sorted, rows);
    }
    const unsigned char* key(size_t r) const { return bytes[rows.model[r]].data() + off[rows.model[r]][rows.index[r]]; }
    size_t keylen(size_t r) const { return (size_t)(off[rows.model[r]][rows.index[r] + 1] - off[rows.model[r]][rows.index[r]]); }
    size_t size() const { return rows.ll.size(); }
};
}  // namespace colibri_host

/** the whole comparison (reference :69-171) in one device call: fills `resultmap` (pattern -> ll) and/or writes the direct output (`-d`: the header
 *  without a newline, then per pattern its text, ll and per model the count and count / tokens() as an int division). Rows come in model order,
 *  then each model's iteration order (the reference's come in its hash maps' order); with `conjunctiononly` only the patterns every model holds. */
inline void comparemodels_loglikelihood(std::vector<PatternModel<uint32_t>*>& models, PatternMap<double>* resultmap, bool conjunctiononly = false,
                                        std::ostream* output = NULL, const ClassDecoder* classdecoder = NULL) {
    colibri_host::CompareBatch b;
    b.run(models, conjunctiononly, false);
    const size_t N = models.size();
    if (output != NULL) {
        *output << "PATTERN\tLOGLIKELIHOOD";
        for (size_t i = 0; i < N; i++) *output << "\tOCC_" << i << "\tFREQ_" << i;
    }
    std::vector<int> total(N);
    for (size_t i = 0; i < N; ++i) total[i] = (int)models[i]->tokens();
    if (resultmap != NULL) resultmap->reserve(resultmap->size() + b.size());
    for (size_t r = 0; r < b.size(); ++r) {
        const double ll = b.rows.ll[r];
        if (resultmap == NULL && (output == NULL || classdecoder == NULL)) break;
        const Pattern pattern(b.key(r), b.keylen(r));
        if (resultmap != NULL) (*resultmap)[pattern] = ll;
        if (output != NULL && classdecoder != NULL) {
            *output << pattern.tostring(*classdecoder) << "\t" << ll;
            for (size_t i = 0; i < N; i++) {
                const int o = (int)b.rows.observed[r * N + i];
                *output << "\t" << o << "\t";
                if (total[i] > 0)
                    *output << o / total[i];
                else
                    *output << 0;
            }
            *output << std::endl;
        }
    }
}
#endif
