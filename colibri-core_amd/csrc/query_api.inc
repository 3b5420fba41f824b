// query_api.inc — part of colibri_hip.hip (included there, inside its extern "C" block, after rindex_api.inc): a pattern model queried with new
// text (colibri-patternmodeller -q / --queryfile; kernels and the specification in query.hpp). The key table and the probe are the constraint
// set's (constrained.hpp), run over position ranges of the query text, which lives in buffers of its own: the context's corpus, its trained
// model and its reference arrays are only read.

// the query text into the query state, tokenised as a corpus is (kernels.hpp: a byte under 128 ends a position, the byte 0 alone is a delimiter)
static int query_text_upload(colibri_ctx* c, DevScratch& S, const uint8_t* payload, uint64_t nbytes) {
    auto& q = c->qy;
    int   rc;
    const size_t padded = ((size_t)nbytes + 15) / 16 * 16 + 64;
    if ((rc = dev_alloc(c, q.bytes, padded))) return rc;
    HIP_TRY(c, hipMemsetAsync(q.bytes.p + nbytes, 0, padded - nbytes, c->stream));
    if (nbytes) HIP_TRY(c, hipMemcpyAsync(q.bytes.p, payload, nbytes, hipMemcpyHostToDevice, c->stream));
    const uint32_t     nblk = std::max<uint32_t>(1, blocks_for(nbytes, kTokBytesPerBlock));
    DevBuf<uint32_t>   blockcnt, total, dcnt, cls;
    DevBuf<CorpusInfo> info;
    if ((rc = S.take(blockcnt, nblk + 1)) || (rc = S.take(total, 1)) || (rc = S.take(info, 1))) return rc;
    hipLaunchKernelGGL(tokenise_count_kernel, dim3(nblk), dim3(kBlock), 0, c->stream, q.bytes.p, nbytes, blockcnt.p);
    hipLaunchKernelGGL(scan_small_kernel, dim3(1), dim3(kBlock), 0, c->stream, blockcnt.p, nblk, total.p);
    uint32_t npos = 0;
    HIP_TRY(c, hipMemcpyAsync(&npos, total.p, sizeof npos, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // (the copy of the caller's text is done too)
    if ((rc = dev_alloc(c, q.tokstart, (size_t)npos + 2)) || (rc = S.take(cls, (size_t)npos + 1))) return rc;
    HIP_TRY(c, hipMemsetAsync(q.tokstart.p, 0, sizeof(uint32_t), c->stream));
    HIP_TRY(c, hipMemsetAsync(info.p, 0, sizeof(CorpusInfo), c->stream));
    const uint32_t pblk = std::max<uint32_t>(1, blocks_for(npos, kBlock));
    if ((rc = S.take(dcnt, pblk + 1))) return rc;
    hipLaunchKernelGGL(tokenise_write_kernel, dim3(nblk), dim3(kBlock), 0, c->stream, q.bytes.p, nbytes, blockcnt.p, q.tokstart.p);
    hipLaunchKernelGGL(position_info_kernel, dim3(pblk), dim3(kBlock), 0, c->stream, q.bytes.p, q.tokstart.p, npos, info.p, dcnt.p, cls.p);
    hipLaunchKernelGGL(scan_small_kernel, dim3(1), dim3(kBlock), 0, c->stream, dcnt.p, pblk, total.p);
    uint32_t   ndelim = 0;
    CorpusInfo hinfo{};
    HIP_TRY(c, hipMemcpyAsync(&ndelim, total.p, sizeof ndelim, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(&hinfo, info.p, sizeof hinfo, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if ((rc = dev_alloc(c, q.delimpos, (size_t)ndelim + 1))) return rc;
    uint32_t last_delim = 0;
    hipLaunchKernelGGL(delimiter_write_kernel, dim3(pblk), dim3(kBlock), 0, c->stream, q.bytes.p, q.tokstart.p, npos, dcnt.p, q.delimpos.p);
    if (ndelim) HIP_TRY(c, hipMemcpyAsync(&last_delim, q.delimpos.p + (ndelim - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    if (hinfo.flags & kFlagTokenTooLong) return fail(c, COLIBRI_ERR_ARG, "query: the text has a token of more than 8 bytes; not a class encoding");
    const uint32_t trailing = ndelim ? npos - (last_delim + 1) : npos;
    q.npos   = npos;
    q.ndelim = ndelim;
    q.nlines = ndelim + (trailing ? 1u : 0u);
    S.drop(blockcnt), S.drop(total), S.drop(info), S.drop(cls), S.drop(dcnt);
    return COLIBRI_OK;
}

// the device pipeline on a model's keys in HBM, np == 0 included
static int query_core(colibri_ctx* c, const ModelView& V, const uint8_t* payload, uint64_t nbytes, uint32_t first_line, const uint8_t* exact, int minlength, int maxlength,
                      uint64_t* nlines_out, uint64_t* nrows_out) {
    auto&          q  = c->qy;
    const uint32_t np = V.np;
    int            rc;
    DevScratch     S{c};
    const uint64_t budget = env_u64("COLIBRI_QUERY_BUDGET", kQueryBudgetBytes);
    const uint64_t hmask  = env_hash_mask("COLIBRI_QUERY_HASH_BITS");  // (tests: a hash of a few bits, so that the byte check decides identity)
    if ((rc = query_text_upload(c, S, payload, nbytes))) return rc;
    const uint32_t npos = q.npos, ndelim = q.ndelim, nlines = q.nlines;
    q.first_line = first_line;
    q.has_exact  = exact != nullptr && nlines != 0;
    if (q.has_exact) {
        if ((rc = dev_alloc(c, q.exact, nlines))) return rc;
        HIP_TRY(c, hipMemcpyAsync(q.exact.p, exact, nlines, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    const uint8_t* dexact = q.has_exact ? q.exact.p : nullptr;
    // the model's longest pattern, in tokens: no longer window or line can be one of its patterns
    uint32_t maxn = 0;
    if (np) {
        DevBuf<uint16_t> ntok;
        DevBuf<uint8_t>  cat;
        uint32_t         G = 0;
        if ((rc = print_pattern_info(c, S, "query", V.kbytes, V.koff, np, ntok, cat, &G))) return rc;
        maxn = G - 1;
        S.drop(ntok);
        S.drop(cat);
    }
    const uint32_t n0 = (uint32_t)std::max(minlength, 1);
    const uint32_t n1 = (uint32_t)std::min<int64_t>(std::max(maxlength, 0), std::min<uint32_t>(maxn, kQueryMaxLine));
    const uint32_t L  = (np && n1 >= n0) ? n1 - n0 + 1 : 0u;
    const uint32_t K  = L + 1;
    const uint64_t ncells = (uint64_t)nlines * K, cap64 = 2ull * np + 1024;
    if (ncells >= 0xFFFFFFF0ull) return fail(c, COLIBRI_ERR_OVERFLOW, "query: %u lines at %u lengths are 2^32 - 16 (line, length) counts or more", nlines, L);
    const uint64_t text  = (uint64_t)nbytes + 80 + 4ull * ((uint64_t)npos + 2) + 4ull * ((uint64_t)ndelim + 1) + nlines;
    const uint64_t fixed = text + 8ull * ((uint64_t)npos + 1) + sizeof(CSlot) * cap64 + 12ull * (ncells + 1) + 12ull * ((uint64_t)nlines + 1) + 4ull * L + 64;
    if (fixed > budget)
        return fail(c, COLIBRI_ERR_OVERFLOW, "query: %u patterns, %u positions and %u lines need %llu bytes, above the budget of %llu bytes (COLIBRI_QUERY_BUDGET)", np, npos, nlines,
                    (unsigned long long)fixed, (unsigned long long)budget);
    const uint64_t per_pos = 16ull * L + 4;  // memb, flags, their scan; posline
    uint64_t       chunk   = env_u64("COLIBRI_QUERY_CHUNK", 0);
    if (chunk == 0) chunk = (budget - fixed) / 2 / per_pos;
    chunk = std::min<uint64_t>(chunk, std::max<uint32_t>(npos, 1u));
    if (L) chunk = std::min<uint64_t>(chunk, 0xFFFFFFF0ull / L - 1);  // (the layers' rows, laid end to end, are one 32-bit-indexed scan)
    if (chunk == 0 || fixed + (chunk + 1) * per_pos > budget)
        return fail(c, COLIBRI_ERR_OVERFLOW, "query: %u lengths over a chunk of positions need %llu bytes per position beside %llu bytes, above the budget of %llu bytes (COLIBRI_QUERY_BUDGET)",
                    L, (unsigned long long)per_pos, (unsigned long long)fixed, (unsigned long long)budget);
    const uint32_t C       = (uint32_t)chunk;
    const uint64_t nchunks = (L && npos) ? ((uint64_t)npos + C - 1) / C : 0;
    const size_t   stride  = (size_t)C + 1;
    const uint32_t cap     = (uint32_t)cap64;
    DevBuf<CSlot>              table;
    DevBuf<uint32_t>           rem, cells, whole, memb, flags, posline, carry, bad;
    DevBuf<unsigned long long> celloff, pref;
    if ((rc = S.take(table, (size_t)cap64)) || (rc = S.take(rem, (size_t)npos + 1)) || (rc = S.take(cells, (size_t)ncells + 1)) || (rc = S.take(celloff, (size_t)ncells + 1)) ||
        (rc = S.take(whole, (size_t)nlines + 1)) || (rc = S.take(carry, (size_t)L + 1)) || (rc = S.take(bad, 1)) || (rc = dev_alloc(c, q.line_off, (size_t)nlines + 1)))
        return rc;
    if (nchunks && ((rc = S.take(memb, (size_t)L * stride)) || (rc = S.take(flags, (size_t)L * stride)) || (rc = S.take(pref, (size_t)L * stride)) || (rc = S.take(posline, stride))))
        return rc;
    HIP_TRY(c, hipMemsetAsync(bad.p, 0, sizeof(uint32_t), c->stream));
    HIP_TRY(c, hipMemsetAsync(cells.p, 0, sizeof(uint32_t) * (ncells + 1), c->stream));
    HIP_TRY(c, hipMemsetAsync(carry.p, 0, sizeof(uint32_t) * ((size_t)L + 1), c->stream));
    {
        Prof p(c, COLIBRI_K_COUNT);
        hipLaunchKernelGGL(constraint_clear_kernel, dim3(stream_grid(cap)), dim3(kBlock), 0, c->stream, table.p, cap);
        if (np) hipLaunchKernelGGL(constraint_insert_kernel, dim3(stream_grid(np)), dim3(kBlock), 0, c->stream, V.kbytes, V.koff, np, table.p, cap, hmask);
        if (npos) hipLaunchKernelGGL(sentence_rem_kernel, dim3(stream_grid(npos)), dim3(kBlock), 0, c->stream, q.delimpos.p, ndelim, npos, rem.p);
        if (nlines)
            hipLaunchKernelGGL(query_whole_kernel, dim3(stream_grid(nlines)), dim3(kBlock), 0, c->stream, q.bytes.p, q.tokstart.p, q.delimpos.p, ndelim, npos, nlines, dexact, table.p, cap,
                               V.kbytes, V.koff, np, maxn, K, hmask, cells.p, whole.p, bad.p);
    }
    uint32_t hbad = 0;
    HIP_TRY(c, hipMemcpyAsync(&hbad, bad.p, sizeof hbad, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    if (hbad & kQueryBadLine) return fail(c, COLIBRI_ERR_OVERFLOW, "query: a line of more than %u tokens (token indices are 16-bit)", kQueryMaxLine);
    // the layers of chunk j, and the scan of their hit flags
    auto layers = [&](uint64_t j, uint32_t& p0, uint32_t& n) -> int {
        p0 = (uint32_t)(j * C), n = std::min<uint32_t>(C, npos - p0);
        {
            Prof p(c, COLIBRI_K_COUNT);
            for (uint32_t l = 0; l < L; l += kProbeLengths)
                hipLaunchKernelGGL(constraint_probe_kernel<false>, dim3(stream_grid(n)), dim3(kBlock), 0, c->stream, q.bytes.p, q.tokstart.p + p0, rem.p + p0, table.p, cap, V.kbytes, V.koff,
                                   n, (int)(n0 + l), (int)std::min<uint32_t>(kProbeLengths, L - l), memb.p + (size_t)l * stride, stride, (const uint32_t*)nullptr, hmask);
        }
        hipLaunchKernelGGL(query_posline_kernel, dim3(stream_grid(n)), dim3(kBlock), 0, c->stream, q.delimpos.p, ndelim, p0, n, posline.p);
        hipLaunchKernelGGL(query_flags_kernel, dim3(stream_grid((uint64_t)L * stride)), dim3(kBlock), 0, c->stream, memb.p, stride, L, n, posline.p, dexact, flags.p);
        return scan_u32(c, flags.p, (uint32_t)((uint64_t)L * stride), pref.p, nullptr);
    };
    uint32_t p0 = 0, n = 0;
    for (uint64_t j = 0; j < nchunks; ++j) {
        if ((rc = layers(j, p0, n))) return rc;
        hipLaunchKernelGGL(query_count_kernel, dim3(stream_grid((uint64_t)L * n)), dim3(kBlock), 0, c->stream, pref.p, stride, L, p0, n, posline.p, q.delimpos.p, ndelim, npos, K, cells.p);
    }
    unsigned long long nrows = 0;
    if (ncells && (rc = scan_u32(c, cells.p, (uint32_t)ncells, celloff.p, &nrows))) return rc;
    if (nrows >= 0xFFFFFFF0ull) return fail(c, COLIBRI_ERR_OVERFLOW, "query: %llu rows (at most 2^32 - 16)", nrows);
    const uint64_t peak = fixed + (nchunks ? (chunk + 1) * per_pos : 0);
    if (peak + 10ull * (nrows + 1) > budget)
        return fail(c, COLIBRI_ERR_OVERFLOW, "query: %llu rows beside %llu bytes of scratch exceed the budget of %llu bytes (COLIBRI_QUERY_BUDGET)", nrows, (unsigned long long)peak,
                    (unsigned long long)budget);
    if ((rc = dev_alloc(c, q.token, (size_t)nrows + 1)) || (rc = dev_alloc(c, q.pattern, (size_t)nrows + 1)) || (rc = dev_alloc(c, q.rowline, (size_t)nrows + 1))) return rc;
    hipLaunchKernelGGL(query_lineoff_kernel, dim3(stream_grid((uint64_t)nlines + 1)), dim3(kBlock), 0, c->stream, celloff.p, nlines, K, nrows, q.line_off.p);
    if (nlines)
        hipLaunchKernelGGL(query_wholefill_kernel, dim3(stream_grid(nlines)), dim3(kBlock), 0, c->stream, cells.p, celloff.p, whole.p, nlines, K, q.token.p, q.pattern.p, q.rowline.p);
    for (uint64_t j = 0; j < nchunks; ++j) {
        if (nchunks > 1 && (rc = layers(j, p0, n))) return rc;  // (a single chunk still holds its layers)
        hipLaunchKernelGGL(query_fill_kernel, dim3(stream_grid((uint64_t)L * n)), dim3(kBlock), 0, c->stream, memb.p, flags.p, pref.p, stride, L, p0, n, posline.p, q.delimpos.p, ndelim, npos,
                           K, celloff.p, carry.p, q.token.p, q.pattern.p, q.rowline.p);
        if (nchunks > 1)
            hipLaunchKernelGGL(query_carry_kernel, dim3(stream_grid(L)), dim3(kBlock), 0, c->stream, pref.p, stride, L, p0, n, posline.p, q.delimpos.p, ndelim, npos, carry.p);
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    collect_events(c);
    q.np       = np;
    q.nrows    = nrows;
    q.chunks   = nchunks;
    q.scratch  = S.peak;
    q.valid    = true;
    *nlines_out = nlines;
    *nrows_out  = nrows;
    return COLIBRI_OK;
}

static int query_begin(colibri_ctx* c, const uint8_t* payload, uint64_t nbytes, uint64_t* nlines, uint64_t* nrows) {
    if (!c || !nlines || !nrows || (!payload && nbytes)) return COLIBRI_ERR_ARG;
    auto& q = c->qy;
    q.valid = false;
    q.nrows = q.chunks = q.windows = q.staging = q.scratch = 0;
    *nlines = *nrows = 0;
    if (nbytes >= 0xFFFFFF00ull) return fail(c, COLIBRI_ERR_OVERFLOW, "query: a text of %llu bytes exceeds 32-bit byte offsets; split it", (unsigned long long)nbytes);
    HIP_TRY(c, hipSetDevice(c->device));
    return COLIBRI_OK;
}

int colibri_query(colibri_ctx* c, const uint64_t* key_off, const uint8_t* key_bytes, const uint32_t* counts, const uint64_t* ref_off, const uint32_t* ref_sentence,
                  const uint16_t* ref_token, uint64_t npatterns, const uint8_t* payload, uint64_t nbytes, uint32_t first_line, const uint8_t* exact, int minlength, int maxlength,
                  uint64_t* nlines, uint64_t* nrows) {
    int rc = query_begin(c, payload, nbytes, nlines, nrows);
    if (rc) return rc;
    ModelView V;
    const unsigned want = (counts || ref_off) ? kModelCounts | kModelOffsets | kModelRefs : 0u;  // neither: the rows can be had, their text cannot
    if ((rc = model_upload(c, "query", key_off, key_bytes, counts, ref_off, ref_sentence, ref_token, npatterns, want, V))) return rc;
    if ((rc = query_core(c, V, payload, nbytes, first_line, exact, minlength, maxlength, nlines, nrows))) return rc;
    auto& q = c->qy;  // the model stays with the result: the text is written from it
    q.resident   = false;
    q.has_counts = counts != nullptr || ref_off != nullptr || npatterns == 0;
    q.has_refs   = V.roff != nullptr;
    q.keybytes   = V.keybytes;
    q.nrefs      = V.nrefs;
    q.kbytes     = std::move(V.own.kbytes);
    q.koff       = std::move(V.own.koff);
    q.cnt        = std::move(V.own.cnt);
    q.roff       = std::move(V.own.roff);
    q.rs         = std::move(V.own.rs);
    q.rt         = std::move(V.own.rt);
    if (!V.cnt) q.cnt.reset();
    return COLIBRI_OK;
}

// the same on the model of the last colibri_train of this context, indexed or not, where it lies in HBM
int colibri_query_resident(colibri_ctx* c, const uint8_t* payload, uint64_t nbytes, uint32_t first_line, const uint8_t* exact, int minlength, int maxlength, uint64_t* nlines,
                           uint64_t* nrows) {
    int rc = query_begin(c, payload, nbytes, nlines, nrows);
    if (rc) return rc;
    ModelView V;
    if ((rc = model_resident(c, "colibri_query_resident", false, V))) return rc;
    if (V.np == 0 && (rc = model_upload(c, "query", nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, V))) return rc;
    if ((rc = query_core(c, V, payload, nbytes, first_line, exact, minlength, maxlength, nlines, nrows))) return rc;
    c->qy.resident   = true;
    c->qy.has_counts = true;
    c->qy.serial     = c->model_serial;
    return COLIBRI_OK;
}

int colibri_query_fetch(colibri_ctx* c, uint64_t* line_off, uint16_t* token, uint32_t* pattern) {
    if (!c) return COLIBRI_ERR_ARG;
    auto& q = c->qy;
    if (!q.valid) return fail(c, COLIBRI_ERR_STATE, "colibri_query / colibri_query_resident first");
    HIP_TRY(c, hipSetDevice(c->device));
    if (line_off) HIP_TRY(c, hipMemcpyAsync(line_off, q.line_off.p, sizeof(uint64_t) * ((size_t)q.nlines + 1), hipMemcpyDeviceToHost, c->stream));
    if (token && q.nrows) HIP_TRY(c, hipMemcpyAsync(token, q.token.p, sizeof(uint16_t) * q.nrows, hipMemcpyDeviceToHost, c->stream));
    if (pattern && q.nrows) HIP_TRY(c, hipMemcpyAsync(pattern, q.pattern.p, sizeof(uint32_t) * q.nrows, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return COLIBRI_OK;
}

// the text of the last query, through output windows and the decoder's pinned double buffers, as print_core hands its windows over
int colibri_query_text(colibri_ctx* c, uint64_t tokens, colibri_decode_sink sink, void* user, uint64_t* outbytes) {
    if (!c || !sink || tokens >= (1ull << 53)) return COLIBRI_ERR_ARG;
    auto& q = c->qy;
    auto& d = c->dc;
    if (outbytes) *outbytes = 0;
    q.windows = q.staging = 0;
    if (!q.valid) return fail(c, COLIBRI_ERR_STATE, "colibri_query_text: colibri_query / colibri_query_resident first");
    if (!q.has_counts) return fail(c, COLIBRI_ERR_STATE, "colibri_query_text: the model was given without counts and reference offsets: its rows cannot be printed");
    if (!c->pr.table) return fail(c, COLIBRI_ERR_STATE, "colibri_query_text: no word table installed by colibri_print_classes");
    HIP_TRY(c, hipSetDevice(c->device));
    int       rc;
    ModelView V;
    if (q.resident) {
        if (!c->trained || c->model_serial != q.serial) return fail(c, COLIBRI_ERR_STATE, "colibri_query_text: the model the query ran on is no longer resident");
        if ((rc = model_resident(c, "colibri_query_text", false, V))) return rc;
    } else {
        V.kbytes = q.kbytes.p, V.koff = q.koff.p, V.cnt = q.cnt.p, V.np = q.np, V.keybytes = q.keybytes, V.nrefs = q.nrefs;
        if (q.has_refs) V.roff = q.roff.p, V.rs = q.rs.p, V.rt = q.rt.p;
    }
    const uint64_t nrows = q.nrows;
    if (nrows == 0) return COLIBRI_OK;
    const uint32_t np = q.np, npos = q.npos, ndelim = q.ndelim;
    DevScratch     S{c};
    const uint64_t budget = env_u64("COLIBRI_QUERY_BUDGET", kQueryBudgetBytes);
    const uint8_t* dexact = q.has_exact ? q.exact.p : nullptr;
    const PrintTable tab{c->pr.wordoff.p, c->pr.words.p, c->pr.has.p, c->pr.nids};
    DevBuf<uint16_t>           ntok;
    DevBuf<uint8_t>            cat, arena, marena;
    DevBuf<unsigned long long> grp, hidx, midx, hroff, CR, arow, moff, rstart;
    DevBuf<uint32_t>           flag, missflag, hitp, refcnt, creflen, head, arowlen, missrow, misslen, rlen, bad;
    DevBuf<PrintRow>           row;
    const uint64_t need0 = 12ull * ((uint64_t)np + 1) + 24ull * (nrows + 1) + 64;
    if (need0 > budget)
        return fail(c, COLIBRI_ERR_OVERFLOW, "query text: %u patterns and %llu rows need %llu bytes of scratch, above the budget of %llu bytes (COLIBRI_QUERY_BUDGET)", np,
                    (unsigned long long)nrows, (unsigned long long)need0, (unsigned long long)budget);
    // (a) the patterns hit at least once and the exact-mode misses, compacted
    if ((rc = S.take(flag, (size_t)np + 1)) || (rc = S.take(hidx, (size_t)np + 1)) || (rc = S.take(missflag, (size_t)nrows + 1)) || (rc = S.take(midx, (size_t)nrows + 1)) ||
        (rc = S.take(bad, 1)))
        return rc;
    HIP_TRY(c, hipMemsetAsync(bad.p, 0, sizeof(uint32_t), c->stream));
    HIP_TRY(c, hipMemsetAsync(flag.p, 0, sizeof(uint32_t) * ((size_t)np + 1), c->stream));
    hipLaunchKernelGGL(query_mark_kernel, dim3(stream_grid(nrows + 1)), dim3(kBlock), 0, c->stream, q.pattern.p, (unsigned long long)nrows, flag.p, missflag.p);
    unsigned long long nh = 0, nmiss = 0, nhrefs = 0, abytes = 0, mbytes = 0, total = 0;
    if ((rc = scan_u32(c, flag.p, np + 1, hidx.p, &nh)) || (rc = scan_u32(c, missflag.p, (uint32_t)nrows + 1, midx.p, &nmiss))) return rc;
    if (nh) {
        // (b) per hit pattern: tokens, category (of the whole model: the groups' totals need every pattern), references, row
        uint32_t G = 0;
        if ((rc = print_pattern_info(c, S, "query text", V.kbytes, V.koff, np, ntok, cat, &G))) return rc;
        const size_t NG = 4 * (size_t)G;
        if ((rc = S.take(grp, 3 * NG))) return rc;
        HIP_TRY(c, hipMemsetAsync(grp.p, 0, sizeof(unsigned long long) * 3 * NG, c->stream));
        {
            const bool lds = 3 * NG * sizeof(unsigned long long) <= 32768;
            hipLaunchKernelGGL(cov_group_kernel, dim3(stream_grid(np)), dim3(kBlock), lds ? 3 * NG * sizeof(unsigned long long) : 0, c->stream, ntok.p, cat.p, V.cnt, V.roff, np, G, (int)lds,
                               grp.p);
        }
        if ((rc = S.take(hitp, (size_t)nh)) || (rc = S.take(refcnt, (size_t)nh + 1)) || (rc = S.take(hroff, (size_t)nh + 1))) return rc;
        hipLaunchKernelGGL(query_compact_kernel, dim3(stream_grid((uint64_t)np + 1)), dim3(kBlock), 0, c->stream, flag.p, hidx.p, np, V.roff, (uint32_t)nh, hitp.p, refcnt.p, bad.p);
        if ((rc = scan_u32(c, refcnt.p, (uint32_t)nh + 1, hroff.p, &nhrefs))) return rc;
        if (nhrefs >= 0xFFFFFFF0ull) return fail(c, COLIBRI_ERR_OVERFLOW, "query text: the patterns found have %llu references (at most 2^32 - 16)", nhrefs);
        if (S.live + 12ull * (nhrefs + 1) > budget)
            return fail(c, COLIBRI_ERR_OVERFLOW, "query text: %llu references of the patterns found exceed the budget of %llu bytes (COLIBRI_QUERY_BUDGET)", nhrefs, (unsigned long long)budget);
        if ((rc = S.take(creflen, (size_t)nhrefs + 1)) || (rc = S.take(CR, (size_t)nhrefs + 1))) return rc;
        if (V.roff) {
            hipLaunchKernelGGL(query_reflen_kernel, dim3(stream_grid(nhrefs + 1)), dim3(kBlock), 0, c->stream, hroff.p, hitp.p, (uint32_t)nh, V.roff, V.rs, V.rt, nhrefs, creflen.p);
            if ((rc = scan_u32(c, creflen.p, (uint32_t)nhrefs + 1, CR.p, nullptr))) return rc;
        }
        if ((rc = S.take(row, (size_t)nh)) || (rc = S.take(head, (size_t)nh)) || (rc = S.take(arowlen, (size_t)nh + 1)) || (rc = S.take(arow, (size_t)nh + 1))) return rc;
        hipLaunchKernelGGL(query_row_kernel, dim3(stream_grid(nh + 1)), dim3(kBlock), 0, c->stream, V.kbytes, V.koff, V.cnt, V.roff, hitp.p, (uint32_t)nh, hroff.p, CR.p, ntok.p, cat.p, G,
                           grp.p + NG, (unsigned long long)tokens, tab, row.p, head.p, arowlen.p, bad.p);
        if ((rc = scan_u32(c, arowlen.p, (uint32_t)nh + 1, arow.p, &abytes))) return rc;
        if (S.live + abytes > budget)
            return fail(c, COLIBRI_ERR_OVERFLOW, "query text: %llu bytes of rows of the patterns found exceed the budget of %llu bytes (COLIBRI_QUERY_BUDGET)", abytes, (unsigned long long)budget);
        if ((rc = S.take(arena, (size_t)abytes + 1))) return rc;
        hipLaunchKernelGGL(query_head_kernel, dim3(stream_grid(nh)), dim3(kBlock), 0, c->stream, V.kbytes, V.koff, V.cnt, V.roff, hitp.p, (uint32_t)nh, ntok.p, cat.p, tab, row.p, arow.p,
                           arena.p);
        if (V.roff && nhrefs)
            hipLaunchKernelGGL(query_refs_kernel, dim3(stream_grid(nhrefs)), dim3(kBlock), 0, c->stream, hroff.p, hitp.p, (uint32_t)nh, V.roff, V.rs, V.rt, CR.p, nhrefs, head.p, arow.p,
                               arena.p);
        S.drop(creflen);
        S.drop(grp);
    }
    S.drop(flag);
    // (c) the NOT FOUND lines
    if ((rc = S.take(missrow, (size_t)nmiss + 1)) || (rc = S.take(misslen, (size_t)nmiss + 1)) || (rc = S.take(moff, (size_t)nmiss + 1))) return rc;
    if (nmiss) {
        hipLaunchKernelGGL(query_miss_len_kernel, dim3(stream_grid(nrows + 1)), dim3(kBlock), 0, c->stream, missflag.p, midx.p, (unsigned long long)nrows, q.rowline.p, q.bytes.p,
                           q.tokstart.p, q.delimpos.p, ndelim, npos, tab, (uint32_t)nmiss, missrow.p, misslen.p, bad.p);
        if ((rc = scan_u32(c, misslen.p, (uint32_t)nmiss + 1, moff.p, &mbytes))) return rc;
        if (S.live + mbytes > budget)
            return fail(c, COLIBRI_ERR_OVERFLOW, "query text: %llu bytes of NOT FOUND lines exceed the budget of %llu bytes (COLIBRI_QUERY_BUDGET)", mbytes, (unsigned long long)budget);
    }
    if ((rc = S.take(marena, (size_t)mbytes + 1))) return rc;
    if (nmiss)
        hipLaunchKernelGGL(query_miss_text_kernel, dim3(stream_grid(nmiss)), dim3(kBlock), 0, c->stream, missrow.p, moff.p, (uint32_t)nmiss, q.rowline.p, q.bytes.p, q.tokstart.p,
                           q.delimpos.p, ndelim, npos, tab, marena.p);
    // (d) the rows' lengths and their scan
    if ((rc = S.take(rlen, (size_t)nrows + 1)) || (rc = S.take(rstart, (size_t)nrows + 1))) return rc;
    hipLaunchKernelGGL(query_rowlen_kernel, dim3(stream_grid(nrows + 1)), dim3(kBlock), 0, c->stream, q.pattern.p, q.token.p, q.rowline.p, (unsigned long long)nrows, dexact, q.first_line,
                       hidx.p, arowlen.p, midx.p, misslen.p, rlen.p, bad.p);
    if ((rc = scan_u32(c, rlen.p, (uint32_t)nrows + 1, rstart.p, &total))) return rc;
    uint32_t hbad = 0;
    HIP_TRY(c, hipMemcpy(&hbad, bad.p, sizeof hbad, hipMemcpyDeviceToHost));
    if (hbad & kQueryBadText) return fail(c, COLIBRI_ERR_OVERFLOW, "query text: a line of 4 GiB or more");
    S.drop(rlen);
    S.drop(missflag);
    // (e) windows of B bytes: the device writes window w into stage[w & 1] and copies it to pinned[w & 1] while the host hands window w - 1 to the sink
    const uint64_t B = std::min<uint64_t>(env_u64("COLIBRI_QUERY_WINDOW_BYTES", kQueryWindowBytes), total);
    if (S.live + 2 * B > budget)
        return fail(c, COLIBRI_ERR_OVERFLOW, "query text: two windows of %llu bytes beside %llu bytes of scratch exceed the budget of %llu bytes (COLIBRI_QUERY_BUDGET)",
                    (unsigned long long)B, (unsigned long long)S.live, (unsigned long long)budget);
    if (d.pinned_n < B) {
        for (auto& p : d.pinned) {
            if (p) (void)hipHostFree(p);
            p = nullptr;
        }
        d.pinned_n = 0;
        for (auto& p : d.pinned) HIP_TRY(c, hipHostMalloc(reinterpret_cast<void**>(&p), B, hipHostMallocDefault));
        d.pinned_n = B;
    }
    for (auto& e : d.ev)
        if (!e) HIP_TRY(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    DevBuf<uint8_t> stage[2];
    if ((rc = S.take(stage[0], B)) || (rc = S.take(stage[1], B))) return rc;
    q.scratch         = std::max<uint64_t>(q.scratch, S.peak);
    const uint64_t nw = (total + B - 1) / B;
    auto hand_over = [&](uint64_t w) -> int {
        HIP_TRY(c, hipEventSynchronize(d.ev[w & 1]));
        const uint64_t n = std::min<uint64_t>(B, total - w * B);
        if (const int s = sink(user, d.pinned[w & 1], n))
            return fail(c, COLIBRI_ERR_STATE, "query text: the sink stopped the call (it returned %d) after %llu bytes", s, (unsigned long long)(w * B));
        return COLIBRI_OK;
    };
    for (uint64_t w = 0; w < nw; ++w) {
        const unsigned long long W0 = w * B, W1 = std::min<uint64_t>(total, W0 + B);
        hipLaunchKernelGGL(query_emit_kernel, dim3(stream_grid((W1 - W0 + kQuerySeg - 1) / kQuerySeg)), dim3(kBlock), 0, c->stream, rstart.p, (unsigned long long)nrows, q.pattern.p,
                           q.token.p, q.rowline.p, dexact, q.first_line, hidx.p, arow.p, arena.p, midx.p, moff.p, marena.p, W0, W1, stage[w & 1].p);
        HIP_TRY(c, hipMemcpyAsync(d.pinned[w & 1], stage[w & 1].p, W1 - W0, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipEventRecord(d.ev[w & 1], c->stream));
        if (w > 0 && (rc = hand_over(w - 1))) {
            (void)hipStreamSynchronize(c->stream);
            return rc;
        }
    }
    if ((rc = hand_over(nw - 1))) return rc;
    HIP_TRY(c, hipGetLastError());
    q.windows = nw;
    q.staging = 2 * B;
    if (outbytes) *outbytes = total;
    return COLIBRI_OK;
}

int colibri_query_info(const colibri_ctx* c, uint64_t* chunks, uint64_t* windows, uint64_t* staging_bytes, uint64_t* scratch_bytes) {
    if (!c) return COLIBRI_ERR_ARG;
    if (chunks) *chunks = c->qy.chunks;
    if (windows) *windows = c->qy.windows;
    if (staging_bytes) *staging_bytes = c->qy.staging;
    if (scratch_bytes) *scratch_bytes = c->qy.scratch;
    return COLIBRI_OK;
}
