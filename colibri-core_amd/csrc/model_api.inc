// model_api.inc — part of colibri_hip.hip (included there ahead of every feature's .inc): what the entry points that take a pattern model share.
// A model reaches a feature's device pipeline (its _core) as one ModelView, built from the caller's host arrays in export layout (model_upload) or
// from the model the last colibri_train left in HBM (model_resident); the scratch accountant and the environment parsers of those pipelines.
namespace {
// scratch accounting of one _core call: `live` / `peak` count the bytes its buffers hold (a drop lowers `live` before the next take; what is
// still held on the way out is freed by the buffers' destructors, which cannot raise the peak)
struct DevScratch {
    colibri_ctx* c;
    uint64_t     live = 0, peak = 0;
    template <class T>
    int take(DevBuf<T>& b, size_t n) {
        const size_t had = b.p ? b.n * sizeof(T) : 0;
        const int    rc  = dev_alloc(c, b, n);
        if (rc) return rc;
        live += b.n * sizeof(T) - had;
        peak = std::max(peak, live);
        return COLIBRI_OK;
    }
    template <class T>
    void drop(DevBuf<T>& b) {
        live -= b.p ? b.n * sizeof(T) : 0;
        b.reset();
    }
};

// a positive integer from the environment, read at each call (budgets, windows, chunks; tests make them small); `dflt` otherwise
uint64_t env_u64(const char* var, uint64_t dflt) {
    const char*     e = getenv(var);
    const long long v = e ? atoll(e) : 0;
    return v > 0 ? (uint64_t)v : dflt;
}
// <var> = <bits> (tests: a hash of a few bits, so that byte checks decide identity): the mask of the low <bits> bits (0 < bits < 64); ~0 otherwise
uint64_t env_hash_mask(const char* var) {
    const uint64_t b = env_u64(var, 0);
    return b > 0 && b < 64 ? (1ull << b) - 1ull : ~0ull;
}

// the key bytes of the resident model into out (c->keybytes bytes; ensure_export first): a gather per segment of the result ids
void gather_key_bytes(colibri_ctx* c, uint8_t* out) {
    Prof p(c, COLIBRI_K_EXPORT);
    for (const auto& sg : c->segments)
        hipLaunchKernelGGL(export_bytes_kernel, dim3(blocks_for(sg.count, kBlock)), dim3(kBlock), 0, c->stream, c->bytes.p, c->tokstart.p, c->res_rep.p, c->keylen.p, c->keyoff.p, sg.first,
                           sg.count, sg.n, sg.mask, out);
}

// a model in HBM as a _core reads it: kbytes (keybytes bytes + 16 zero bytes of slack) / koff (np + 1), cnt (np counts, or NULL: the number of
// references), roff (np + 1) / rs / rt (nrefs references; roff == NULL: an unindexed model, nrefs == 0). np == 0: nothing else is set.
struct ModelView {
    const uint8_t*            kbytes = nullptr;
    const unsigned long long* koff   = nullptr;
    const uint32_t*           cnt    = nullptr;
    const unsigned long long* roff   = nullptr;
    const uint32_t*           rs     = nullptr;
    const uint16_t*           rt     = nullptr;
    uint32_t                  np     = 0;
    uint64_t                  keybytes = 0, nrefs = 0;
    struct {  // what the view allocated itself; pointers into the context's arrays are borrowed
        DevBuf<uint8_t>            kbytes;
        DevBuf<unsigned long long> koff, roff;
        DevBuf<uint32_t>           cnt, rs;
        DevBuf<uint16_t>           rt;
    } own;
};

// the parts of a loaded model a caller takes beside its keys
enum : unsigned {
    kModelCounts  = 1,  // the counts, when given (with kModelOffsets: they or the offsets must be)
    kModelOffsets = 2,  // the reference offsets, when given
    kModelRefs    = 4,  // and with the offsets the references
    kModelNeedOffsets = 8,  // the offsets must be given
    kModelIndexed = kModelNeedOffsets | kModelOffsets | kModelRefs,
};

// a model in export layout from the host into HBM. The caller's arrays may go once this returns.
int model_upload(colibri_ctx* c, const char* what, const uint64_t* key_off, const uint8_t* key_bytes, const uint32_t* counts, const uint64_t* ref_off, const uint32_t* ref_sentence,
                 const uint16_t* ref_token, uint64_t npatterns, unsigned want, ModelView& v) {
    if (!(want & kModelCounts)) counts = nullptr;
    if (!(want & kModelOffsets)) ref_off = nullptr;
    if (npatterns && (!key_off || !key_bytes)) return COLIBRI_ERR_ARG;
    if ((want & kModelNeedOffsets) && !ref_off) return COLIBRI_ERR_ARG;
    if ((want & kModelCounts) && (want & kModelOffsets) && !counts && !ref_off) return COLIBRI_ERR_ARG;
    const bool     refs  = ref_off && (want & kModelRefs);
    const uint64_t nb_in = npatterns ? key_off[npatterns] : 0, nr_in = ref_off ? ref_off[npatterns] : 0;
    if (refs && nr_in && (!ref_sentence || !ref_token)) return COLIBRI_ERR_ARG;
    if (npatterns >= 0x7FFFFFF0ull || nr_in >= 0xFFFFFFF0ull)
        return fail(c, COLIBRI_ERR_OVERFLOW, "%s: %llu patterns / %llu references exceed 32-bit indexing", what, (unsigned long long)npatterns, (unsigned long long)nr_in);
    HIP_TRY(c, hipSetDevice(c->device));
    const uint32_t np = (uint32_t)npatterns;
    auto&          o  = v.own;
    int            rc;
    if ((rc = dev_alloc(c, o.kbytes, (size_t)nb_in + 16)) || (rc = dev_alloc(c, o.koff, (size_t)np + 1))) return rc;
    HIP_TRY(c, hipMemsetAsync(o.kbytes.p + nb_in, 0, 16, c->stream));  // (the key readers fetch whole words: the slack after the last key is defined)
    if (nb_in) HIP_TRY(c, hipMemcpyAsync(o.kbytes.p, key_bytes, nb_in, hipMemcpyHostToDevice, c->stream));
    if (np) HIP_TRY(c, hipMemcpyAsync(o.koff.p, key_off, sizeof(uint64_t) * ((size_t)np + 1), hipMemcpyHostToDevice, c->stream));
    if (counts && np) {
        if ((rc = dev_alloc(c, o.cnt, np))) return rc;
        HIP_TRY(c, hipMemcpyAsync(o.cnt.p, counts, sizeof(uint32_t) * np, hipMemcpyHostToDevice, c->stream));
    }
    if (ref_off) {
        if ((rc = dev_alloc(c, o.roff, (size_t)np + 1))) return rc;
        HIP_TRY(c, hipMemcpyAsync(o.roff.p, ref_off, sizeof(uint64_t) * ((size_t)np + 1), hipMemcpyHostToDevice, c->stream));
    }
    if (refs) {
        if ((rc = dev_alloc(c, o.rs, (size_t)nr_in + 1)) || (rc = dev_alloc(c, o.rt, (size_t)nr_in + 1))) return rc;
        if (nr_in) {
            HIP_TRY(c, hipMemcpyAsync(o.rs.p, ref_sentence, sizeof(uint32_t) * nr_in, hipMemcpyHostToDevice, c->stream));
            HIP_TRY(c, hipMemcpyAsync(o.rt.p, ref_token, sizeof(uint16_t) * nr_in, hipMemcpyHostToDevice, c->stream));
        }
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // (the copies read the caller's pageable memory: none is left enqueued, whatever the _core does next)
    v.kbytes = o.kbytes.p, v.koff = o.koff.p, v.cnt = o.cnt.p, v.roff = o.roff.p, v.rs = o.rs.p, v.rt = o.rt.p;
    v.np = np, v.keybytes = nb_in, v.nrefs = nr_in;
    return COLIBRI_OK;
}

// the model of the last colibri_train of this context where it lies in HBM (`what`: the entry point, for the messages); need_indexed: an
// unindexed model is refused. A trained model of no patterns leaves v.np == 0. Nothing of the context's state is written.
int model_resident(colibri_ctx* c, const char* what, bool need_indexed, ModelView& v) {
    if (need_indexed && (!c->trained || !c->opt.indexed || c->sh.active)) return fail(c, COLIBRI_ERR_STATE, "%s needs the indexed model of a colibri_train on this context", what);
    if (!c->trained || c->sh.active) return fail(c, COLIBRI_ERR_STATE, "%s needs the model of a colibri_train on this context (not a sharded run)", what);
    if (c->seeded_model) return fail(c, COLIBRI_ERR_STATE, "%s: the result of a seeded run is only the part of the expanded model that occurs in the corpus; merge it and pass the model in", what);
    const uint32_t R       = c->hstate.res_total;
    const bool     indexed = c->opt.indexed != 0;
    if (R == 0) return COLIBRI_OK;
    if (indexed && c->npairs >= 0xFFFFFFF0ull) return fail(c, COLIBRI_ERR_OVERFLOW, "%s: %llu references exceed 32-bit indexing", what, (unsigned long long)c->npairs);
    HIP_TRY(c, hipSetDevice(c->device));
    int rc;
    if ((rc = ensure_export(c))) return rc;  // key lengths / offsets of the resident model
    if ((rc = dev_alloc(c, v.own.kbytes, (size_t)c->keybytes + 16))) return rc;
    HIP_TRY(c, hipMemsetAsync(v.own.kbytes.p + c->keybytes, 0, 16, c->stream));
    gather_key_bytes(c, v.own.kbytes.p);
    v.kbytes = v.own.kbytes.p, v.koff = c->keyoff.p, v.cnt = c->res_cnt.p;
    v.np = R, v.keybytes = c->keybytes;
    if (indexed) {  // reference offsets = the exclusive scan of the counts (an indexed model's count is its number of references), closed by their number
        const unsigned long long nr_total = c->npairs;
        if ((rc = dev_alloc(c, v.own.roff, (size_t)R + 1)) || (rc = scan_u32(c, c->res_cnt.p, R, v.own.roff.p, nullptr))) return rc;
        HIP_TRY(c, hipMemcpyAsync(v.own.roff.p + R, &nr_total, sizeof nr_total, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));  // the host word above is read by the copy
        v.roff = v.own.roff.p, v.rs = c->ref_sentence.p, v.rt = c->ref_token.p, v.nrefs = c->npairs;
    }
    return COLIBRI_OK;
}
}  // namespace
