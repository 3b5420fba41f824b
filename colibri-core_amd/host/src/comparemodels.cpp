// colibri-comparemodels (MI355X build) — a drop-in for the reference's model comparison (src/comparemodels.cpp): the log-likelihood of every
// pattern across two or more models (Rayson & Garside 2000), sorted by it, or written directly (-d). Same options, output and exit codes;
// -N, which the reference lists but does not parse (it aborts on it), is refused with a message. The whole comparison is one device call
// (colibri_compare); this file parses options, loads the models and prints.
#include <getopt.h>

#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "patternmodel.h"

namespace {

void usage() {
    std::cerr << "colibri-comparemodels (MI355X-native build of the Colibri Core model comparison)\n"
                 "Syntax: colibri-comparemodels -c classfile patternmodelfile1 patternmodelfile2 etc...\n"
                 "Description: Compares the frequency of patterns between two or more pattern models by computing log likelihood, following the methodology of "
                 "Rayson and Garside (2000), Comparing corpora using frequency profiling. In proceedings of the workshop on Comparing Corpora, held in conjunction "
                 "with the 38th annual meeting of the Association for Computational Linguistics (ACL 2000). 1-8 October 2000, Hong Kong, pp. 1 - 6\n\n"
                 "Important notes: - All models should be full models, and best generated with the same occurrence threshold, rather than constrained train/test models!\n"
                 "                 - Models must share the exact same class encoding to be comparable!\n"
                 "Options:\n"
                 "\t-l int   Maximum pattern length (default unlimited)\n"
                 "\t-m int   Minimum pattern length (default 1)\n"
                 "\t-S       omit skipgrams\n"
                 "\t-F       omit flexgrams\n"
                 "\t-a       Include only patterns that occur in all models\n"
                 "\t-d       Output directly, don't build a map, don't sort the output (conserves memory)\n"
                 "The log-likelihood of every pattern is computed on the GPU (one call over all models)."
              << std::endl;
}

}  // namespace

int main(int argc, char* argv[]) {
    std::string              classfile;
    std::vector<std::string> modelfiles;
    bool                     conjunctiononly = false, directoutput = false;
    PatternModelOptions      options;
    int                      c;
    while ((c = getopt(argc, argv, "c:hl:m:NSFad")) != -1) {
        switch (c) {
            case 'c': classfile = optarg; break;
            case 'l': options.MAXLENGTH = atoi(optarg); break;
            case 'm': options.MINLENGTH = atoi(optarg); break;
            case 'N':
                std::cerr << "ERROR: -N (omit n-grams) is not an option of colibri-comparemodels (the reference lists it but does not parse it)" << std::endl;
                return 2;
            case 'S': options.DOREMOVESKIPGRAMS = true; break;
            case 'F': options.DOREMOVEFLEXGRAMS = true; break;
            case 'a': conjunctiononly = true; break;
            case 'd': directoutput = true; break;
            case 'h': usage(); return 0;
            default: std::cerr << "ERROR: Unknown option: -" << (char)optopt << std::endl; return 2;
        }
    }
    for (int i = optind; i < argc; ++i) modelfiles.push_back(argv[i]);
    if (classfile.empty()) {
        std::cerr << "ERROR: No class file specified! (-c)" << std::endl;
        usage();
        return 2;
    }
    if (modelfiles.size() < 2) {
        std::cerr << "ERROR: Need at least two models" << std::endl;
        usage();
        return 2;
    }
    try {
        const ClassDecoder                   classdecoder(classfile);
        std::vector<PatternModel<uint32_t>*> models;
        struct Owner {
            std::vector<PatternModel<uint32_t>*>& m;
            ~Owner() {
                for (auto* p : m) delete p;
            }
        } owner{models};
        for (const auto& filename : modelfiles) {
            std::cerr << "Loading model " << filename << std::endl;
            models.push_back(new PatternModel<uint32_t>(filename, options));
        }
        std::cerr << "Computing log-likelihood..." << std::endl;
        if (directoutput) {
            PatternMap<double> llmodel;
            comparemodels_loglikelihood(models, &llmodel, conjunctiononly, &std::cout, &classdecoder);
            return 0;
        }
        colibri_host::CompareBatch b;
        b.run(models, conjunctiononly, true);  // rows already in the reference's (-ll, Pattern) order
        std::cerr << "Sorting results..." << std::endl;
        std::cerr << "Output:" << std::endl;
        const size_t N = models.size();
        std::cout << "PATTERN\tLOGLIKELIHOOD";
        for (size_t i = 0; i < N; ++i) std::cout << "\tOCC_" << i << "\tFREQ_" << i;
        std::cout << "\n";
        for (size_t r = 0; r < b.size(); ++r) {
            const double key = -1 * b.rows.ll[r];  // (the reference prints the negated sort key negated again: 0 for -0)
            std::cout << Pattern(b.key(r), b.keylen(r)).tostring(classdecoder) << "\t" << (key * -1);
            for (size_t i = 0; i < N; ++i) {
                const unsigned int o = b.rows.observed[r * N + i];
                std::cout << "\t" << o << "\t" << o / (double)b.rows.group_totals[r * N + i];  // frequency(): count / (double)totaloccurrencesingroup(category, n)
            }
            std::cout << "\n";
        }
        std::cout.flush();
        return 0;
    } catch (const std::exception& e) {
        std::cerr << "colibri-comparemodels: " << e.what() << std::endl;
        return 1;
    }
}
