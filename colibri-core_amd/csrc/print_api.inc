// print_api.inc — part of colibri_hip.hip (included there, inside its extern "C" block, after coverage_api.inc): the text and the histogram of a
// pattern model (colibri-patternmodeller -P [--instantiate] / -H; kernels and the specification in print.hpp).

int colibri_print_classes(colibri_ctx* c, const uint64_t* word_off, const uint8_t* word_bytes, const uint8_t* has_word, uint64_t nids) {
    if (!c || !word_off) return COLIBRI_ERR_ARG;
    auto& p = c->pr;
    p.nids  = 0;
    p.table = false;
    if (nids > kDecodeMaxIds)
        return fail(c, COLIBRI_ERR_OVERFLOW, "print: a word table of %llu ids exceeds the bound of %u ids (the highest id that can have a word is %u)", (unsigned long long)nids,
                    kDecodeMaxIds, kDecodeMaxIds - 1);
    if (!word_bytes && word_off[nids] > word_off[0]) return COLIBRI_ERR_ARG;
    std::vector<uint32_t> off32(nids + 1, 0);
    std::vector<uint8_t>  has(nids + 1, 1);
    for (uint64_t k = 1; k <= nids; ++k) {
        if (word_off[k] < word_off[k - 1]) return fail(c, COLIBRI_ERR_ARG, "print: word offsets decrease at id %llu", (unsigned long long)k);
        if (word_off[k] - word_off[0] >= 0xFFFFFFFFull) return fail(c, COLIBRI_ERR_OVERFLOW, "print: the words take 4 GiB or more (32-bit offsets)");
        off32[k] = (uint32_t)(word_off[k] - word_off[0]);
    }
    if (has_word) std::copy(has_word, has_word + nids, has.begin());
    HIP_TRY(c, hipSetDevice(c->device));
    int rc;
    if ((rc = dev_alloc(c, p.wordoff, nids + 1)) || (rc = dev_alloc(c, p.words, (size_t)off32[nids] + 1)) || (rc = dev_alloc(c, p.has, nids + 1))) return rc;
    HIP_TRY(c, hipMemcpyAsync(p.wordoff.p, off32.data(), sizeof(uint32_t) * (nids + 1), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(p.has.p, has.data(), nids + 1, hipMemcpyHostToDevice, c->stream));
    if (off32[nids]) HIP_TRY(c, hipMemcpyAsync(p.words.p, word_bytes + word_off[0], off32[nids], hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // (the caller's arrays may go once this returns)
    p.nids  = (uint32_t)nids;
    p.table = true;
    return COLIBRI_OK;
}

// per pattern: tokens and category (cov_info_kernel); a pattern of more than 65535 tokens or a token of more than kCovMaxToken bytes is refused
static int print_pattern_info(colibri_ctx* c, DevScratch& S, const char* what, const uint8_t* kbytes, const unsigned long long* koff, uint32_t np, DevBuf<uint16_t>& ntok,
                              DevBuf<uint8_t>& cat, uint32_t* G) {
    int                        rc;
    DevBuf<unsigned long long> info;
    if ((rc = S.take(ntok, np)) || (rc = S.take(cat, np)) || (rc = S.take(info, 2))) return rc;
    HIP_TRY(c, hipMemsetAsync(info.p, 0, 2 * sizeof(unsigned long long), c->stream));
    hipLaunchKernelGGL(cov_info_kernel, dim3(stream_grid(np)), dim3(kBlock), 0, c->stream, kbytes, koff, np, ntok.p, cat.p, info.p);
    unsigned long long hinfo[2];
    HIP_TRY(c, hipMemcpyAsync(hinfo, info.p, sizeof hinfo, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    S.drop(info);
    if (hinfo[0] > 0xFFFFull) return fail(c, COLIBRI_ERR_OVERFLOW, "%s: a pattern of %llu tokens (at most 65535)", what, hinfo[0]);
    if (hinfo[1] == ~0ull) return fail(c, COLIBRI_ERR_OVERFLOW, "%s: a token of more than %u bytes", what, kCovMaxToken);
    *G = (uint32_t)hinfo[0] + 1;
    return COLIBRI_OK;
}

// the device pipeline on a model in HBM, indexed or not
// inst: with instances (colibri_print_instances): behind every reference of a skipgram row the corpus text found there, from the context's corpus. Only an
// indexed model has any; the two per-reference kernels change, the scratch does not grow (the emit looks a reference's pattern up again).
static int print_core(colibri_ctx* c, const ModelView& V, uint64_t tokens, colibri_decode_sink sink, void* user, uint64_t* outbytes, bool inst = false) {
    const uint32_t np    = V.np;
    const uint64_t nrefs = V.nrefs;
    auto&          p = c->pr;
    auto&          d = c->dc;  // (the pinned staging and its events are the decoder's: one pair per context)
    int            rc;
    DevScratch     S{c};
    const uint64_t budget = env_u64("COLIBRI_PRINT_BUDGET", kPrintBudgetBytes);
    const uint32_t slice  = (uint32_t)std::min<uint64_t>(env_u64("COLIBRI_PRINT_SLICE", kPrintSlice), 1u << 20);
    const uint64_t need = (uint64_t)np * (2 + 1 + sizeof(PrintRow) + 4 + 4 + 8) + nrefs * 12 + 64;
    if (need > budget)
        return fail(c, COLIBRI_ERR_OVERFLOW, "print: %u patterns and %llu references need %llu bytes of scratch, above the budget of %llu bytes (COLIBRI_PRINT_BUDGET)", np,
                    (unsigned long long)nrefs, (unsigned long long)need, (unsigned long long)budget);
    DevBuf<uint16_t>           ntok;
    DevBuf<uint8_t>            cat;
    DevBuf<unsigned long long> grp, R, rowstart;
    DevBuf<uint32_t>           reflen, head, rowlen, bad, range;
    DevBuf<PrintRow>           row;
    uint32_t                   G = 0;
    // (a) per pattern: tokens, category; (b) the groups' occurrence totals. No reference is read for either.
    if ((rc = print_pattern_info(c, S, "print", V.kbytes, V.koff, np, ntok, cat, &G))) return rc;
    const size_t NG = 4 * (size_t)G;
    if ((rc = S.take(grp, 3 * NG))) return rc;
    HIP_TRY(c, hipMemsetAsync(grp.p, 0, sizeof(unsigned long long) * 3 * NG, c->stream));
    {
        const bool lds = 3 * NG * sizeof(unsigned long long) <= 32768;
        hipLaunchKernelGGL(cov_group_kernel, dim3(stream_grid(np)), dim3(kBlock), lds ? 3 * NG * sizeof(unsigned long long) : 0, c->stream, ntok.p, cat.p, V.cnt, V.roff, np, G, (int)lds,
                           grp.p);
    }
    inst = inst && V.roff;  // (an unindexed model prints as colibri_print_model prints it)
    const PrintTable  tab{p.wordoff.p, p.words.p, p.has.p, p.nids};
    const PrintCorpus cor{c->bytes.p, c->tokstart.p, c->delimpos.p, c->ndelim, c->npos, c->ndelim + 1, c->first_sentence};  // (the positions after the last delimiter form sentence ndelim, possibly empty)
    if (inst) {  // a flexgram among the keys: category 3's all-sizes group has patterns
        unsigned long long flex = 0;
        HIP_TRY(c, hipMemcpyAsync(&flex, grp.p + 3 * (size_t)G, sizeof flex, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (flex)
            return fail(c, COLIBRI_ERR_UNSUPPORTED, "print with instances: the model holds %llu flexgrams, which are not instantiated (the reference's walk accepts gaps of exactly one token)", flex);
    }
    // (c) the references' lengths and their scan
    if (V.roff) {
        if ((rc = S.take(reflen, (size_t)nrefs + 1)) || (rc = S.take(R, (size_t)nrefs + 1))) return rc;
        if (inst) {
            DevBuf<uint32_t> badref;
            uint32_t         hbadref = 0;
            if ((rc = S.take(badref, 1))) return rc;
            HIP_TRY(c, hipMemsetAsync(badref.p, 0, sizeof(uint32_t), c->stream));
            hipLaunchKernelGGL(print_instlen_kernel, dim3((uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(blocks_for(nrefs, slice), 256ull * 16))), dim3(kBlock), 0, c->stream, V.roff, V.rs,
                               V.rt, ntok.p, cat.p, np, nrefs, slice, cor, tab, reflen.p, badref.p);
            HIP_TRY(c, hipMemcpyAsync(&hbadref, badref.p, sizeof hbadref, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            HIP_TRY(c, hipGetLastError());
            S.drop(badref);
            if (hbadref & kPrintBadRef)
                return fail(c, COLIBRI_ERR_ARG, "print with instances: a skipgram's reference does not fit the corpus (its sentence is not among the %u from %u on, or ends before the pattern does): is this the model's corpus?",
                            c->ndelim + 1, c->first_sentence);
            if (hbadref & kPrintBadRow) return fail(c, COLIBRI_ERR_OVERFLOW, "print: a row of 4 GiB or more");
        } else {
            hipLaunchKernelGGL(print_reflen_kernel, dim3(stream_grid(nrefs + 1)), dim3(kBlock), 0, c->stream, V.rs, V.rt, nrefs, reflen.p);
        }
        if ((rc = scan_u32(c, reflen.p, (uint32_t)nrefs + 1, R.p, nullptr))) return rc;
    }
    // (d) the rows: the doubles, the heads, the lengths and their scan
    if ((rc = S.take(row, np)) || (rc = S.take(head, np)) || (rc = S.take(rowlen, (size_t)np + 1)) || (rc = S.take(rowstart, (size_t)np + 1)) || (rc = S.take(bad, 1)) ||
        (rc = S.take(range, 4)))
        return rc;
    HIP_TRY(c, hipMemsetAsync(bad.p, 0, sizeof(uint32_t), c->stream));
    hipLaunchKernelGGL(print_row_kernel, dim3(stream_grid((uint64_t)np + 1)), dim3(kBlock), 0, c->stream, V.kbytes, V.koff, V.cnt, V.roff, R.p, ntok.p, cat.p, np, G, grp.p + NG,
                       (unsigned long long)tokens, tab, row.p, head.p, rowlen.p, bad.p);
    unsigned long long total = 0;
    if ((rc = scan_u32(c, rowlen.p, np + 1, rowstart.p, &total))) return rc;
    uint32_t hbad = 0;
    HIP_TRY(c, hipMemcpy(&hbad, bad.p, sizeof hbad, hipMemcpyDeviceToHost));
    if (hbad & kPrintBadRow) return fail(c, COLIBRI_ERR_OVERFLOW, "print: a row of 4 GiB or more");
    S.drop(reflen);
    S.drop(rowlen);
    S.drop(grp);
    p.scratch = S.peak;
    // (e) windows of B bytes: the device writes window w into stage[w & 1] and copies it to pinned[w & 1] while the host hands window w - 1 to the sink
    const uint64_t B = std::min<uint64_t>(env_u64("COLIBRI_PRINT_WINDOW_BYTES", kPrintWindowBytes), total);
    if (need + 2 * B > budget)
        return fail(c, COLIBRI_ERR_OVERFLOW, "print: two windows of %llu bytes beside %llu bytes of scratch exceed the budget of %llu bytes (COLIBRI_PRINT_BUDGET)",
                    (unsigned long long)B, (unsigned long long)need, (unsigned long long)budget);
    if (d.pinned_n < B) {
        for (auto& q : d.pinned) {
            if (q) (void)hipHostFree(q);
            q = nullptr;
        }
        d.pinned_n = 0;
        for (auto& q : d.pinned) HIP_TRY(c, hipHostMalloc(reinterpret_cast<void**>(&q), B, hipHostMallocDefault));
        d.pinned_n = B;
    }
    for (auto& e : d.ev)
        if (!e) HIP_TRY(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    DevBuf<uint8_t> stage[2];
    if ((rc = S.take(stage[0], B)) || (rc = S.take(stage[1], B))) return rc;
    p.scratch         = S.peak;
    const uint64_t nw = (total + B - 1) / B;
    auto hand_over = [&](uint64_t w) -> int {
        HIP_TRY(c, hipEventSynchronize(d.ev[w & 1]));
        const uint64_t n = std::min<uint64_t>(B, total - w * B);
        if (const int s = sink(user, d.pinned[w & 1], n))
            return fail(c, COLIBRI_ERR_STATE, "print: the sink stopped the call (it returned %d) after %llu bytes", s, (unsigned long long)(w * B));
        return COLIBRI_OK;
    };
    const uint32_t ref_grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(blocks_for(std::min<uint64_t>(nrefs, B), slice) + 2, 256ull * 16));  // (a window of B bytes holds fewer than B references)
    for (uint64_t w = 0; w < nw; ++w) {
        const unsigned long long W0 = w * B, W1 = std::min<uint64_t>(total, W0 + B);
        hipLaunchKernelGGL(print_range_kernel, dim3(1), dim3(kWave), 0, c->stream, rowstart.p, head.p, V.roff, R.p, np, W0, W1, range.p);
        hipLaunchKernelGGL(print_head_kernel, dim3(stream_grid(std::min<uint64_t>(np, B + 1))), dim3(kBlock), 0, c->stream, V.kbytes, V.koff, V.cnt, V.roff, ntok.p, cat.p, tab, row.p, head.p,
                           rowstart.p, range.p, W0, W1, stage[w & 1].p);
        if (V.roff && nrefs && inst)
            hipLaunchKernelGGL(print_insts_kernel, dim3(ref_grid), dim3(kBlock), 0, c->stream, V.roff, V.rs, V.rt, R.p, head.p, rowstart.p, ntok.p, cat.p, np, slice, range.p, cor, tab, W0, W1,
                               stage[w & 1].p);
        else if (V.roff && nrefs)
            hipLaunchKernelGGL(print_refs_kernel, dim3(ref_grid), dim3(kBlock), 0, c->stream, V.roff, V.rs, V.rt, R.p, head.p, rowstart.p, np, slice, range.p, W0, W1, stage[w & 1].p);
        HIP_TRY(c, hipMemcpyAsync(d.pinned[w & 1], stage[w & 1].p, W1 - W0, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipEventRecord(d.ev[w & 1], c->stream));
        if (w > 0 && (rc = hand_over(w - 1))) {
            (void)hipStreamSynchronize(c->stream);
            return rc;
        }
    }
    if ((rc = hand_over(nw - 1))) return rc;
    HIP_TRY(c, hipGetLastError());
    p.windows = nw;
    p.staging = 2 * B;
    if (outbytes) *outbytes = total;
    return COLIBRI_OK;
}

static int print_begin(colibri_ctx* c, uint64_t tokens, colibri_decode_sink sink, uint64_t* outbytes) {
    if (!c || !sink || tokens >= (1ull << 53)) return COLIBRI_ERR_ARG;
    c->pr.windows = c->pr.staging = c->pr.scratch = 0;
    if (outbytes) *outbytes = 0;
    if (!c->pr.table) return fail(c, COLIBRI_ERR_STATE, "print: no word table installed by colibri_print_classes");
    return COLIBRI_OK;
}

int colibri_print_model(colibri_ctx* c, const uint64_t* key_off, const uint8_t* key_bytes, const uint32_t* counts, const uint64_t* ref_off, const uint32_t* ref_sentence,
                        const uint16_t* ref_token, uint64_t npatterns, uint64_t tokens, colibri_decode_sink sink, void* user, uint64_t* outbytes) {
    int rc = print_begin(c, tokens, sink, outbytes);
    if (rc || npatterns == 0) return rc;
    ModelView V;
    if ((rc = model_upload(c, "print", key_off, key_bytes, counts, ref_off, ref_sentence, ref_token, npatterns, kModelCounts | kModelOffsets | kModelRefs, V))) return rc;
    return print_core(c, V, tokens, sink, user, outbytes);
}

int colibri_print_model_resident(colibri_ctx* c, uint64_t tokens, colibri_decode_sink sink, void* user, uint64_t* outbytes) {
    int rc = print_begin(c, tokens, sink, outbytes);
    if (rc) return rc;
    ModelView V;
    if ((rc = model_resident(c, "colibri_print_model_resident", false, V)) || V.np == 0) return rc;
    return print_core(c, V, tokens, sink, user, outbytes);
}

// with instances: the context's corpus is the one the references point into
static int print_instances_begin(colibri_ctx* c, uint64_t tokens, colibri_decode_sink sink, uint64_t* outbytes) {
    const int rc = print_begin(c, tokens, sink, outbytes);
    if (rc) return rc;
    if (!c->have_corpus) return fail(c, COLIBRI_ERR_STATE, "print with instances: no corpus uploaded (colibri_upload_corpus)");
    return COLIBRI_OK;
}

int colibri_print_instances(colibri_ctx* c, const uint64_t* key_off, const uint8_t* key_bytes, const uint32_t* counts, const uint64_t* ref_off, const uint32_t* ref_sentence,
                            const uint16_t* ref_token, uint64_t npatterns, uint64_t tokens, colibri_decode_sink sink, void* user, uint64_t* outbytes) {
    int rc = print_instances_begin(c, tokens, sink, outbytes);
    if (rc || npatterns == 0) return rc;
    ModelView V;
    if ((rc = model_upload(c, "print", key_off, key_bytes, counts, ref_off, ref_sentence, ref_token, npatterns, kModelCounts | kModelOffsets | kModelRefs, V))) return rc;
    return print_core(c, V, tokens, sink, user, outbytes, true);
}

int colibri_print_instances_resident(colibri_ctx* c, uint64_t tokens, colibri_decode_sink sink, void* user, uint64_t* outbytes) {
    int rc = print_instances_begin(c, tokens, sink, outbytes);
    if (rc) return rc;
    ModelView V;
    if ((rc = model_resident(c, "colibri_print_instances_resident", false, V)) || V.np == 0) return rc;
    return print_core(c, V, tokens, sink, user, outbytes, true);
}

int colibri_print_info(const colibri_ctx* c, uint64_t* windows, uint64_t* staging_bytes, uint64_t* scratch_bytes) {
    if (!c) return COLIBRI_ERR_ARG;
    if (windows) *windows = c->pr.windows;
    if (staging_bytes) *staging_bytes = c->pr.staging;
    if (scratch_bytes) *scratch_bytes = c->pr.scratch;
    return COLIBRI_OK;
}

// ---- histogram -------------------------------------------------------------------------------------------------------------------------------
static int hist_core(colibri_ctx* c, const ModelView& V, int category, uint32_t size, uint64_t* nrows) {
    const uint32_t             np = V.np;
    auto&                      p = c->pr;
    int                        rc;
    DevScratch                 S{c};
    DevBuf<uint16_t>           ntok;
    DevBuf<uint8_t>            cat;
    DevBuf<uint32_t>           flag, key[2], val[2], value, start;
    DevBuf<unsigned long long> pos;
    if (category || size) {
        uint32_t G = 0;
        if ((rc = print_pattern_info(c, S, "histogram", V.kbytes, V.koff, np, ntok, cat, &G))) return rc;
    }
    if ((rc = S.take(flag, np)) || (rc = S.take(pos, np)) || (rc = S.take(key[0], np)) || (rc = S.take(key[1], np)) || (rc = S.take(val[0], np)) || (rc = S.take(val[1], np))) return rc;
    hipLaunchKernelGGL(hist_select_kernel, dim3(stream_grid(np)), dim3(kBlock), 0, c->stream, ntok.p, cat.p, np, (uint32_t)category, size, flag.p);
    unsigned long long m = 0;
    if ((rc = scan_u32(c, flag.p, np, pos.p, &m))) return rc;
    if (m) {
        hipLaunchKernelGGL(hist_gather_kernel, dim3(stream_grid(np)), dim3(kBlock), 0, c->stream, V.cnt, V.roff, flag.p, pos.p, np, key[0].p);
        HIP_TRY(c, hipMemsetAsync(val[0].p, 0, sizeof(uint32_t) * m, c->stream));
        uint32_t* const k2[2] = {key[0].p, key[1].p};
        uint32_t* const v2[2] = {val[0].p, val[1].p};
        int             cur   = 0;
        if ((rc = radix_sort_pairs(c, k2, v2, m, 32, cur))) return rc;
        hipLaunchKernelGGL(hist_heads_kernel, dim3(stream_grid(m)), dim3(kBlock), 0, c->stream, k2[cur], (uint32_t)m, flag.p);
        unsigned long long rows = 0;
        if ((rc = scan_u32(c, flag.p, (uint32_t)m, pos.p, &rows))) return rc;
        if ((rc = S.take(value, rows)) || (rc = S.take(start, rows))) return rc;
        hipLaunchKernelGGL(hist_rows_kernel, dim3(stream_grid(m)), dim3(kBlock), 0, c->stream, k2[cur], flag.p, pos.p, (uint32_t)m, value.p, start.p);
        p.hcount.assign(rows, 0);
        std::vector<uint32_t> hstart(rows + 1, 0);
        HIP_TRY(c, hipMemcpyAsync(p.hcount.data(), value.p, sizeof(uint32_t) * rows, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(hstart.data(), start.p, sizeof(uint32_t) * rows, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        HIP_TRY(c, hipGetLastError());
        hstart[rows] = (uint32_t)m;
        p.hpatterns.assign(rows, 0);
        for (size_t j = 0; j < rows; ++j) p.hpatterns[j] = hstart[j + 1] - hstart[j];
    }
    p.scratch = S.peak;
    p.hvalid  = true;
    *nrows    = p.hcount.size();
    return COLIBRI_OK;
}

static int hist_begin(colibri_ctx* c, int category, uint64_t size, uint64_t* nrows) {
    if (!c || !nrows || category < 0 || category > 3 || size > 0xFFFFFFFFull) return COLIBRI_ERR_ARG;
    c->pr.hvalid = false;
    c->pr.hcount.clear();
    c->pr.hpatterns.clear();
    *nrows = 0;
    return COLIBRI_OK;
}

int colibri_histogram(colibri_ctx* c, const uint64_t* key_off, const uint8_t* key_bytes, const uint32_t* counts, const uint64_t* ref_off, uint64_t npatterns, int category,
                      uint64_t size, uint64_t* nrows) {
    int rc = hist_begin(c, category, size, nrows);
    if (rc) return rc;
    if (npatterns == 0) {
        c->pr.hvalid = true;
        return COLIBRI_OK;
    }
    ModelView V;
    if ((rc = model_upload(c, "histogram", key_off, key_bytes, counts, ref_off, nullptr, nullptr, npatterns, kModelCounts | kModelOffsets, V))) return rc;
    return hist_core(c, V, category, (uint32_t)size, nrows);
}

int colibri_histogram_resident(colibri_ctx* c, int category, uint64_t size, uint64_t* nrows) {
    int rc = hist_begin(c, category, size, nrows);
    if (rc) return rc;
    ModelView V;
    if ((rc = model_resident(c, "colibri_histogram_resident", false, V))) return rc;
    if (V.np == 0) {
        c->pr.hvalid = true;
        return COLIBRI_OK;
    }
    return hist_core(c, V, category, (uint32_t)size, nrows);
}

int colibri_histogram_fetch(colibri_ctx* c, uint32_t* counts, uint64_t* patterns) {
    if (!c) return COLIBRI_ERR_ARG;
    const auto& p = c->pr;
    if (!p.hvalid) return fail(c, COLIBRI_ERR_STATE, "colibri_histogram / colibri_histogram_resident first");
    if (counts) std::copy(p.hcount.begin(), p.hcount.end(), counts);
    if (patterns) std::copy(p.hpatterns.begin(), p.hpatterns.end(), patterns);
    return COLIBRI_OK;
}
