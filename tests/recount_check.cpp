// recount_check — test driver (tests/test_recount.py compiles and runs it): PatternModel::trainskipgrams_selfconstrained on a loaded model,
// as colibri-patternmodeller -I -s reaches it after the n-gram rebuild, but on its own, so that the host route (COLIBRI_RECOUNT=host) runs
// without a device.
//   recount_check <model> <corpus> i|u <mintokens> <firstsentence>
// loads the model with DORESET under the threshold, with the corpus attached, calls the routine, and prints one line per skipgram left:
//   <hex key> TAB <count> TAB <sentence:token> ...   (an unindexed model: no third column)
// then "minmax <minlength> <maxlength> hasskipgrams <0|1>".
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>

#include "patternmodel.h"

static std::string refs_of(const uint32_t&) { return std::string(); }
static std::string refs_of(const IndexedData& d) {
    std::string out;
    for (const IndexReference& r : d.data) {
        if (!out.empty()) out += " ";
        out += r.tostring();
    }
    return out;
}

template <class Model>
static int run(Model& model, const std::string& modelfile, PatternModelOptions& options, uint32_t firstsentence, bool indexed) {
    model.load(modelfile, options);
    model.trainskipgrams_selfconstrained(options, firstsentence);
    for (typename Model::iterator it = model.begin(); it != model.end(); ++it) {
        if (it->first.category() != SKIPGRAM) continue;
        std::cout << it->first.tohex() << "\t" << model.occurrencecount(it->first);
        if (indexed) std::cout << "\t";
        std::cout << refs_of(it->second) << "\n";
    }
    std::cout << "minmax " << model.minlength() << " " << model.maxlength() << " hasskipgrams " << (model.hasskipgrams() ? 1 : 0) << std::endl;
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 6) {
        std::fprintf(stderr, "usage: recount_check <model> <corpus> i|u <mintokens> <firstsentence>\n");
        return 2;
    }
    const std::string   modelfile = argv[1], corpusfile = argv[2];
    const bool          indexed = argv[3][0] == 'i';
    PatternModelOptions options;
    options.MINTOKENS = std::atoi(argv[4]);
    options.DORESET   = true;
    options.QUIET     = true;
    const uint32_t firstsentence = (uint32_t)std::atoi(argv[5]);
    try {
        IndexedCorpus corpus(corpusfile);
        if (indexed) {
            IndexedPatternModel<> model(&corpus);
            return run(model, modelfile, options, firstsentence, true);
        }
        PatternModel<uint32_t> model(&corpus);
        return run(model, modelfile, options, firstsentence, false);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "recount_check: %s\n", e.what());
        return 1;
    }
}
