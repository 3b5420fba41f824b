// relations_api.inc — part of colibri_hip.hip (included there, inside its extern "C" block, after cooc_api.inc): pattern relations of an
// indexed model (colibri-patternmodeller --subsumes / --subsumed / --leftneighbours / --rightneighbours, and getinstances / gettemplates; kernels
// and the specification in relations.hpp). The pipeline is cooc_core's with a relation kind.

static int relations_begin(colibri_ctx* c, int kind, uint64_t* nrows) {
    if (!c || !nrows || kind < COLIBRI_REL_SUBCHILDREN || kind > COLIBRI_REL_TEMPLATES) return COLIBRI_ERR_ARG;
    auto& rl = c->rl;
    rl.valid = false;
    rl.nrows = rl.events = rl.scratch = 0;
    rl.chunks = 0;
    *nrows    = 0;
    if (!c->have_corpus) return fail(c, COLIBRI_ERR_STATE, "relations need the corpus uploaded (colibri_upload_corpus): it is the reverse index");
    return COLIBRI_OK;
}

int colibri_relations(colibri_ctx* c, const uint64_t* key_off, const uint8_t* key_bytes, const uint64_t* ref_off, const uint32_t* ref_sentence, const uint16_t* ref_token,
                      uint64_t npatterns, int kind, uint32_t threshold, uint64_t* nrows) {
    int rc = relations_begin(c, kind, nrows);
    if (rc) return rc;
    if (npatterns == 0) {
        c->rl.valid = true;
        return COLIBRI_OK;
    }
    ModelView V;
    if ((rc = model_upload(c, "relations", key_off, key_bytes, nullptr, ref_off, ref_sentence, ref_token, npatterns, kModelIndexed, V))) return rc;
    return cooc_core(c, V, threshold, 0, 0.0, nrows, kind);
}

int colibri_relations_resident(colibri_ctx* c, int kind, uint32_t threshold, uint64_t* nrows) {
    int rc = relations_begin(c, kind, nrows);
    if (rc) return rc;
    ModelView V;
    if ((rc = model_resident(c, "colibri_relations_resident", true, V))) return rc;
    if (V.np == 0) {
        c->rl.valid = true;
        return COLIBRI_OK;
    }
    return cooc_core(c, V, threshold, 0, 0.0, nrows, kind);
}

int colibri_relations_fetch(colibri_ctx* c, uint32_t* pattern_a, uint32_t* pattern_b, uint32_t* counts) {
    if (!c) return COLIBRI_ERR_ARG;
    auto& rl = c->rl;
    if (!rl.valid) return fail(c, COLIBRI_ERR_STATE, "colibri_relations / colibri_relations_resident first");
    const uint64_t K = rl.nrows;
    if (!K) return COLIBRI_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    if (pattern_a) HIP_TRY(c, hipMemcpyAsync(pattern_a, rl.a.p, sizeof(uint32_t) * K, hipMemcpyDeviceToHost, c->stream));
    if (pattern_b) HIP_TRY(c, hipMemcpyAsync(pattern_b, rl.b.p, sizeof(uint32_t) * K, hipMemcpyDeviceToHost, c->stream));
    if (counts) HIP_TRY(c, hipMemcpyAsync(counts, rl.cnt.p, sizeof(uint32_t) * K, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return COLIBRI_OK;
}

int colibri_relations_info(const colibri_ctx* c, uint64_t* events, uint64_t* chunks, uint64_t* scratch_bytes) {
    if (!c) return COLIBRI_ERR_ARG;
    if (events) *events = c->rl.events;
    if (chunks) *chunks = c->rl.chunks;
    if (scratch_bytes) *scratch_bytes = c->rl.scratch;
    return COLIBRI_OK;
}
