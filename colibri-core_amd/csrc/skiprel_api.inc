// skiprel_api.inc — part of colibri_hip.hip (included there, inside its extern "C" block, after relations_api.inc): the skip content of an
// indexed model's skipgrams (colibri-patternmodeller --skipcontent; kernels and the specification in skiprel.hpp). The identity of a content is
// decided here; counting and ordering are cooc_core's.
extern "C++" {
namespace {
// every reference with a content gets the number of its (A, content) pair; the distinct pairs' facts and bytes (see skiprel.hpp)
int skc_identity(colibri_ctx* c, DevScratch& S, const RelArgs& r, uint64_t nrefs, SkcHook& H) {
    int            rc;
    const uint64_t hmask = env_hash_mask("COLIBRI_SKC_HASH_BITS");  // (tests: a hash of a few bits, so that the byte checks and the further rounds decide)
    DevBuf<uint32_t>           flag, rep, pend[2], slot_of, carry, word;
    DevBuf<unsigned long long> at, skipped;
    DevBuf<FSlot>              table;
    if ((rc = S.take(H.cnum, (size_t)nrefs + 1)) || (rc = S.take(flag, (size_t)nrefs + 1)) || (rc = S.take(rep, (size_t)nrefs + 1)) || (rc = S.take(at, (size_t)nrefs + 1)) ||
        (rc = S.take(skipped, 1)) || (rc = S.take(word, 1)))
        return rc;
    HIP_TRY(c, hipMemsetAsync(skipped.p, 0, sizeof(unsigned long long), c->stream));
    HIP_TRY(c, hipMemsetAsync(word.p, 0, sizeof(uint32_t), c->stream));
    HIP_TRY(c, hipMemsetAsync(flag.p + nrefs, 0, sizeof(uint32_t), c->stream));
    unsigned long long npend = 0;
    {
        Prof p(c, COLIBRI_K_EMIT);
        hipLaunchKernelGGL(skc_flag_kernel, dim3(stream_grid(nrefs)), dim3(kBlock), 0, c->stream, r, nrefs, flag.p, rep.p, skipped.p);
    }
    if ((rc = scan_u32(c, flag.p, (uint32_t)nrefs + 1, at.p, &npend))) return rc;
    unsigned long long hskipped = 0;
    HIP_TRY(c, hipMemcpyAsync(&hskipped, skipped.p, sizeof hskipped, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    H.skipped = hskipped;
    H.rounds  = 0;
    if (npend) {
        const uint64_t cap64 = 2ull * npend + 1024;  // (a slot per distinct hash at most: the probe always meets a free slot)
        if (cap64 > 0xFFFFFFFFull) return fail(c, COLIBRI_ERR_OVERFLOW, "skipcontent: %llu references with a content exceed the identity table", (unsigned long long)npend);
        for (int i = 0; i < 2; ++i)
            if ((rc = S.take(pend[i], (size_t)npend + 1))) return rc;
        if ((rc = S.take(slot_of, (size_t)npend + 1)) || (rc = S.take(carry, (size_t)npend + 1)) || (rc = S.take(table, (size_t)cap64))) return rc;
        hipLaunchKernelGGL(skc_pend_kernel, dim3(stream_grid(nrefs)), dim3(kBlock), 0, c->stream, flag.p, at.p, nrefs, pend[0].p);
        int cur = 0;
        while (npend) {  // every round numbers at least the class of the lowest pending reference of each slot
            const uint32_t cap = (uint32_t)std::min<uint64_t>(cap64, 2ull * npend + 1024);
            Prof           p(c, COLIBRI_K_COUNT);
            hipLaunchKernelGGL(flex_clear_kernel, dim3(stream_grid(cap)), dim3(kBlock), 0, c->stream, table.p, cap);
            hipLaunchKernelGGL(skc_insert_kernel, dim3(stream_grid(npend)), dim3(kBlock), 0, c->stream, r, pend[cur].p, (uint64_t)npend, (uint32_t)H.rounds, hmask, table.p, cap, slot_of.p);
            hipLaunchKernelGGL(skc_resolve_kernel, dim3(stream_grid(npend)), dim3(kBlock), 0, c->stream, r, pend[cur].p, (uint64_t)npend, table.p, slot_of.p, rep.p, carry.p);
            HIP_TRY(c, hipMemsetAsync(carry.p + npend, 0, sizeof(uint32_t), c->stream));
            unsigned long long left = 0;
            if ((rc = scan_u32(c, carry.p, (uint32_t)npend + 1, at.p, &left))) return rc;  // (synchronises: `left` is on the host)
            ++H.rounds;
            if (left >= npend) return fail(c, COLIBRI_ERR_OVERFLOW, "skipcontent: an identity round numbered nothing");
            if (left) hipLaunchKernelGGL(skc_carry_kernel, dim3(stream_grid(npend)), dim3(kBlock), 0, c->stream, pend[cur].p, carry.p, at.p, (uint64_t)npend, pend[cur ^ 1].p);
            cur ^= 1;
            npend = left;
        }
        for (int i = 0; i < 2; ++i) S.drop(pend[i]);
        S.drop(slot_of);
        S.drop(carry);
        S.drop(table);
    }
    // the representatives numbered in reference order
    unsigned long long nd = 0;
    hipLaunchKernelGGL(skc_isrep_kernel, dim3(stream_grid(nrefs)), dim3(kBlock), 0, c->stream, rep.p, nrefs, flag.p);
    HIP_TRY(c, hipMemsetAsync(flag.p + nrefs, 0, sizeof(uint32_t), c->stream));
    if ((rc = scan_u32(c, flag.p, (uint32_t)nrefs + 1, at.p, &nd))) return rc;
    H.nd = nd;
    if ((rc = S.take(H.da, (size_t)nd + 1)) || (rc = S.take(H.dsrc, (size_t)nd + 1)) || (rc = S.take(H.dlen, (size_t)nd + 1)) || (rc = S.take(H.dpb, (size_t)nd + 1)) ||
        (rc = S.take(H.doff, (size_t)nd + 1)))
        return rc;
    HIP_TRY(c, hipMemsetAsync(H.dlen.p + nd, 0, sizeof(uint32_t), c->stream));
    hipLaunchKernelGGL(skc_number_kernel, dim3(stream_grid(nrefs)), dim3(kBlock), 0, c->stream, r, rep.p, at.p, nrefs, H.cnum.p, H.da.p, H.dsrc.p, H.dlen.p, H.dpb.p, word.p);
    unsigned long long nbytes = 0;
    if ((rc = scan_u32(c, H.dlen.p, (uint32_t)nd + 1, H.doff.p, &nbytes))) return rc;
    HIP_TRY(c, hipMemcpyAsync(&H.maxlen, word.p, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if ((rc = S.take(H.dbytes, (size_t)nbytes + 16))) return rc;
    hipLaunchKernelGGL(skc_bytes_kernel, dim3(stream_grid(nd)), dim3(kBlock), 0, c->stream, c->bytes.p, H.dsrc.p, (const uint32_t*)nullptr, H.doff.p, (uint64_t)nd, H.dbytes.p);
    S.drop(flag);
    S.drop(rep);
    S.drop(at);
    return COLIBRI_OK;
}
// cooc_core's rows (A, pair number, count) into c->sk: the content's model number, the contents' bytes in row order
int skc_finish(colibri_ctx* c, SkcHook& H, uint64_t* nrows, uint64_t* content_bytes) {
    auto&          sk = c->sk;
    const uint64_t K  = H.rows.nrows;
    int            rc;
    DevBuf<uint32_t> len;
    if ((rc = dev_alloc(c, sk.pb, (size_t)K + 1)) || (rc = dev_alloc(c, sk.off, (size_t)K + 1)) || (rc = dev_alloc(c, len, (size_t)K + 1))) return rc;
    unsigned long long nbytes = 0;
    HIP_TRY(c, hipMemsetAsync(len.p + K, 0, sizeof(uint32_t), c->stream));
    if (K) hipLaunchKernelGGL(skc_rows_kernel, dim3(stream_grid(K)), dim3(kBlock), 0, c->stream, H.rows.b.p, K, H.dpb.p, H.dlen.p, sk.pb.p, len.p);
    if ((rc = scan_u32(c, len.p, (uint32_t)K + 1, sk.off.p, &nbytes))) return rc;
    if ((rc = dev_alloc(c, sk.bytes, (size_t)nbytes + 16))) return rc;
    if (K) hipLaunchKernelGGL(skc_bytes_kernel, dim3(stream_grid(K)), dim3(kBlock), 0, c->stream, c->bytes.p, H.dsrc.p, (const uint32_t*)H.rows.b.p, sk.off.p, K, sk.bytes.p);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    sk.a             = std::move(H.rows.a);
    sk.cnt           = std::move(H.rows.cnt);
    sk.nrows         = K;
    sk.content_bytes = nbytes;
    sk.events        = H.rows.events;
    sk.chunks        = H.rows.chunks;
    sk.scratch       = H.rows.scratch;
    sk.rounds        = H.rounds;
    sk.skipped       = H.skipped;
    sk.valid         = true;
    *nrows           = K;
    if (content_bytes) *content_bytes = nbytes;
    return COLIBRI_OK;
}
}  // namespace
}  // extern "C++"

static int skipcontent_begin(colibri_ctx* c, uint64_t* nrows, uint64_t* content_bytes) {
    if (!c || !nrows) return COLIBRI_ERR_ARG;
    auto& sk = c->sk;
    sk.valid = false;
    sk.nrows = sk.content_bytes = sk.events = sk.chunks = sk.scratch = sk.rounds = sk.skipped = 0;
    *nrows = 0;
    if (content_bytes) *content_bytes = 0;
    if (!c->have_corpus) return fail(c, COLIBRI_ERR_STATE, "skipcontent needs the corpus uploaded (colibri_upload_corpus): the contents are slices of it");
    return COLIBRI_OK;
}

int colibri_skipcontent(colibri_ctx* c, const uint64_t* key_off, const uint8_t* key_bytes, const uint64_t* ref_off, const uint32_t* ref_sentence, const uint16_t* ref_token,
                        uint64_t npatterns, uint64_t* nrows, uint64_t* content_bytes) {
    int rc = skipcontent_begin(c, nrows, content_bytes);
    if (rc) return rc;
    if (npatterns == 0) {
        c->sk.valid = true;
        return COLIBRI_OK;
    }
    ModelView V;
    SkcHook   H;
    uint64_t  n = 0;
    if ((rc = model_upload(c, "skipcontent", key_off, key_bytes, nullptr, ref_off, ref_sentence, ref_token, npatterns, kModelIndexed, V))) return rc;
    if ((rc = cooc_core(c, V, 0, 0, 0.0, &n, kRelInstances, &H))) return rc;
    return skc_finish(c, H, nrows, content_bytes);
}

int colibri_skipcontent_resident(colibri_ctx* c, uint64_t* nrows, uint64_t* content_bytes) {
    int rc = skipcontent_begin(c, nrows, content_bytes);
    if (rc) return rc;
    ModelView V;
    if ((rc = model_resident(c, "colibri_skipcontent_resident", true, V))) return rc;
    if (V.np == 0) {
        c->sk.valid = true;
        return COLIBRI_OK;
    }
    SkcHook  H;
    uint64_t n = 0;
    if ((rc = cooc_core(c, V, 0, 0, 0.0, &n, kRelInstances, &H))) return rc;
    return skc_finish(c, H, nrows, content_bytes);
}

int colibri_skipcontent_fetch(colibri_ctx* c, uint32_t* pattern_a, uint32_t* pattern_b, uint32_t* counts, uint64_t* content_off, uint8_t* content_bytes) {
    if (!c) return COLIBRI_ERR_ARG;
    auto& sk = c->sk;
    if (!sk.valid) return fail(c, COLIBRI_ERR_STATE, "colibri_skipcontent / colibri_skipcontent_resident first");
    const uint64_t K = sk.nrows;
    if (!K) {
        if (content_off) content_off[0] = 0;
        return COLIBRI_OK;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    if (pattern_a) HIP_TRY(c, hipMemcpyAsync(pattern_a, sk.a.p, sizeof(uint32_t) * K, hipMemcpyDeviceToHost, c->stream));
    if (pattern_b) HIP_TRY(c, hipMemcpyAsync(pattern_b, sk.pb.p, sizeof(uint32_t) * K, hipMemcpyDeviceToHost, c->stream));
    if (counts) HIP_TRY(c, hipMemcpyAsync(counts, sk.cnt.p, sizeof(uint32_t) * K, hipMemcpyDeviceToHost, c->stream));
    if (content_off) HIP_TRY(c, hipMemcpyAsync(content_off, sk.off.p, sizeof(uint64_t) * (K + 1), hipMemcpyDeviceToHost, c->stream));
    if (content_bytes && sk.content_bytes) HIP_TRY(c, hipMemcpyAsync(content_bytes, sk.bytes.p, sk.content_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return COLIBRI_OK;
}

int colibri_skipcontent_info(const colibri_ctx* c, uint64_t* events, uint64_t* chunks, uint64_t* scratch_bytes, uint64_t* rounds, uint64_t* skipped_refs) {
    if (!c) return COLIBRI_ERR_ARG;
    if (events) *events = c->sk.events;
    if (chunks) *chunks = c->sk.chunks;
    if (scratch_bytes) *scratch_bytes = c->sk.scratch;
    if (rounds) *rounds = c->sk.rounds;
    if (skipped_refs) *skipped_refs = c->sk.skipped;
    return COLIBRI_OK;
}
