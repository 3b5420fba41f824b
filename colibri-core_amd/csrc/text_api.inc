// text_api.inc — part of colibri_hip.hip (included there, inside its extern "C" block): colibri_set_constraint (SURVEY §8 f-3)
// and the colibri_text_* entry points of the class encoder (SURVEY §8 f-2).
// constrained training (SURVEY §8 f-3, constrained.hpp): the pattern set the next colibri_train calls are restricted to
int colibri_set_constraint(colibri_ctx* c, const uint64_t* key_off, const uint8_t* key_bytes, uint64_t npatterns) {
    if (!c) return COLIBRI_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    auto& cs = c->cs;
    cs.n     = 0;
    cs.continuation = false;
    cs.filter       = false;
    cs.seed = cs.seed_open = cs.seed_ran = false;
    cs.shapes.clear();
    cs.orders[0] = cs.orders[1] = 0;
    if (npatterns == 0) return COLIBRI_OK;
    if (!key_off || !key_bytes) return COLIBRI_ERR_ARG;
    if (npatterns >= 0x7FFFFFF0ull) return fail(c, COLIBRI_ERR_OVERFLOW, "constraint set too large");
    int            rc;
    const uint64_t nbytes = key_off[npatterns];
    const uint64_t cap64  = 2 * npatterns + 1024;
    if ((rc = dev_alloc(c, cs.bytes, (size_t)nbytes + 16)) || (rc = dev_alloc(c, cs.off, (size_t)npatterns + 1)) || (rc = dev_alloc(c, cs.table, (size_t)cap64))) return rc;
    cs.cap = (uint32_t)cap64;
    HIP_TRY(c, hipMemcpyAsync(cs.bytes.p, key_bytes, nbytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(cs.off.p, key_off, sizeof(uint64_t) * (npatterns + 1), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(constraint_clear_kernel, dim3(stream_grid(cs.cap)), dim3(kBlock), 0, c->stream, cs.table.p, cs.cap);
    hipLaunchKernelGGL(constraint_insert_kernel, dim3(stream_grid(npatterns)), dim3(kBlock), 0, c->stream, cs.bytes.p, cs.off.p, (uint32_t)npatterns, cs.table.p, cs.cap, ~0ull);
    // is the set prefix-closed (a model built with the look-back is)? Then the membership probe may stop at a position's first miss.
    DevBuf<uint32_t> open_flag;
    if ((rc = dev_alloc(c, open_flag, 1))) return rc;
    HIP_TRY(c, hipMemsetAsync(open_flag.p, 0, sizeof(uint32_t), c->stream));
    hipLaunchKernelGGL(constraint_closed_kernel, dim3(stream_grid(npatterns)), dim3(kBlock), 0, c->stream, cs.bytes.p, cs.off.p, (uint32_t)npatterns, cs.table.p, cs.cap, open_flag.p);
    uint32_t is_open = 1;
    HIP_TRY(c, hipMemcpyAsync(&is_open, open_flag.p, sizeof is_open, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    cs.closed = !is_open;
    cs.n      = (uint32_t)npatterns;
    return COLIBRI_OK;
}

int colibri_set_continuation(colibri_ctx* c, const uint64_t* key_off, const uint8_t* key_bytes, uint64_t npatterns) {
    int rc = colibri_set_constraint(c, key_off, key_bytes, npatterns);
    if (rc || npatterns == 0) return rc;
    auto& cs = c->cs;
    for (uint64_t p = 0; p < npatterns; ++p) {  // which orders does the model have n-grams of (cache_grouptotal[NGRAM][n] > 0, patternmodel.h:986)
        uint32_t ntok = 0;
        bool     gap  = false;
        for (uint64_t k = key_off[p]; k < key_off[p + 1]; ++k) {
            const bool first = k == key_off[p] || key_bytes[k - 1] < 128;
            if (key_bytes[k] < 128) {
                ++ntok;
                if (first && (key_bytes[k] == 3 || key_bytes[k] == 4)) gap = true;  // skip class 03 / flex class 04 (classencoder.h:61-62): a skipgram / flexgram, not an n-gram of its length
            }
        }
        if (!gap && ntok >= 1 && ntok < 128) cs.orders[ntok >> 6] |= 1ull << (ntok & 63);
    }
    cs.continuation = true;
    return COLIBRI_OK;
}

int colibri_set_filter(colibri_ctx* c, const uint64_t* key_off, const uint8_t* key_bytes, uint64_t npatterns) {
    int rc = colibri_set_constraint(c, key_off, key_bytes, npatterns);
    if (rc || npatterns == 0) return rc;
    auto& cs = c->cs;
    for (uint64_t p = 0; p < npatterns; ++p) {  // the lengths of the set's n-grams and the (length, gap mask) shapes of its skipgrams; a flexgram matches nothing (src/pattern.cpp:1768-1771)
        uint32_t ntok = 0, mask = 0;
        bool     flex = false;
        for (uint64_t k = key_off[p]; k < key_off[p + 1]; ++k) {
            const bool first = k == key_off[p] || key_bytes[k - 1] < 128;
            if (key_bytes[k] < 128) {
                if (first && key_bytes[k] == 3 && ntok < 31) mask |= 1u << ntok;
                if (first && key_bytes[k] == 4) flex = true;
                ++ntok;
            }
        }
        if (flex || ntok < 1 || ntok >= 128) continue;
        if (mask == 0) {
            cs.orders[ntok >> 6] |= 1ull << (ntok & 63);
        } else if (ntok <= (uint32_t)kMaskedMaxTokens) {
            const std::pair<int, uint32_t> shape((int)ntok, mask);
            if (std::find(cs.shapes.begin(), cs.shapes.end(), shape) == cs.shapes.end()) cs.shapes.push_back(shape);
        } else {
            cs.n = 0;
            return fail(c, COLIBRI_ERR_UNSUPPORTED, "filter: skipgrams of more than 13 tokens are not on the accelerated path");
        }
    }
    cs.filter = true;
    return COLIBRI_OK;
}

// =====================================================================================================================
// class encoder (SURVEY §8 f-2; kernels in textenc.hpp). The host side of the boundary decides the class of every DISTINCT word
// (colibri-core_amd/host: ClassEncoder — the tie order among equally frequent words is the reference's container order and is
// reproduced there); the device does everything that is proportional to the corpus.
// =====================================================================================================================
int colibri_text_upload(colibri_ctx* c, const uint8_t* text, uint64_t nbytes) {
    if (!c || (!text && nbytes)) return COLIBRI_ERR_ARG;
    if (nbytes >= 0x7FFFFFF0ull) return fail(c, COLIBRI_ERR_CORPUS, "text of %llu bytes: at most 2 GiB per call", (unsigned long long)nbytes);
    HIP_TRY(c, hipSetDevice(c->device));
    auto& t = c->tx;
    int   rc;
    if ((rc = dev_alloc(c, t.text, (size_t)nbytes + 16)) || (rc = dev_alloc(c, t.info, 1)) || (rc = dev_alloc(c, t.state, 1)) || (rc = dev_alloc(c, t.ntok, 1))) return rc;
    t.n       = (uint32_t)nbytes;
    t.rules   = -1;
    t.encoded = false;
    if (nbytes) HIP_TRY(c, hipMemcpyAsync(t.text.p, text, nbytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(t.info.p, 0, sizeof(TextInfo), c->stream));
    if (nbytes) hipLaunchKernelGGL(text_info_kernel, dim3(stream_grid(nbytes)), dim3(kBlock), 0, c->stream, t.text.p, t.n, t.info.p);
    HIP_TRY(c, hipMemcpyAsync(&t.hinfo, t.info.p, sizeof(TextInfo), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    // the event list (segment starts and newlines, in text order) every later pass walks
    t.nevents = t.hinfo.nsegments + t.hinfo.nlines;
    if (t.nevents) {
        const uint32_t nblk = blocks_for(nbytes, kEvBytesPerBlock), nb = std::max<uint32_t>(1, blocks_for(nblk, kBlock * 4));
        if ((rc = dev_alloc(c, t.events, (size_t)t.nevents + 1)) || (rc = dev_alloc(c, t.evcnt, (size_t)nblk + 1)) || (rc = dev_alloc(c, t.outoff, (size_t)nblk + 1)) ||
            (rc = dev_alloc(c, t.bsum, (size_t)nb + 1)))
            return rc;
        hipLaunchKernelGGL(text_event_count_kernel, dim3(nblk), dim3(kBlock), 0, c->stream, t.text.p, t.n, t.evcnt.p);
        hipLaunchKernelGGL(scan_reduce_kernel, dim3(nb), dim3(kBlock), 0, c->stream, t.evcnt.p, nblk, t.bsum.p);
        hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(kBlock), 0, c->stream, t.bsum.p, nb, t.bsum.p + nb);
        hipLaunchKernelGGL(scan_apply_kernel, dim3(nb), dim3(kBlock), 0, c->stream, t.evcnt.p, nblk, t.bsum.p, t.outoff.p);
        hipLaunchKernelGGL(text_event_write_kernel, dim3(nblk), dim3(kBlock), 0, c->stream, t.text.p, t.n, t.outoff.p, t.events.p);
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        HIP_TRY(c, hipGetLastError());
    }
    return COLIBRI_OK;
}

int colibri_text_count(colibri_ctx* c, int rules, uint64_t* nwords, uint64_t* ndistinct) {
    if (!c) return COLIBRI_ERR_ARG;
    auto& t   = c->tx;
    // the count below rewrites the table and the word arrays: whatever way it ends other than COLIBRI_OK, nothing of an earlier count is
    // left for colibri_text_words / colibri_text_encode to read
    t.rules   = -1;
    t.encoded = false;
    if (!nwords || !ndistinct || (rules != 0 && rules != 1)) return COLIBRI_ERR_ARG;
    if (!t.text.p) return fail(c, COLIBRI_ERR_STATE, "colibri_text_upload first");
    HIP_TRY(c, hipSetDevice(c->device));
    int            rc;
    const uint64_t cap64 = (uint64_t)t.hinfo.nsegments + (t.hinfo.nsegments >> 1) + 1024;
    t.cap               = (uint32_t)cap64;
    if ((rc = dev_alloc(c, t.table, t.cap)) || (rc = dev_alloc(c, t.slot_of, (size_t)t.nevents + 1)) || (rc = dev_alloc(c, t.first, t.cap)) || (rc = dev_alloc(c, t.widx, t.cap)) ||
        (rc = dev_alloc(c, t.wstart, (size_t)t.hinfo.nsegments + 1)) || (rc = dev_alloc(c, t.wlen, (size_t)t.hinfo.nsegments + 1)) ||
        (rc = dev_alloc(c, t.wcount, (size_t)t.hinfo.nsegments + 1)))
        return rc;
    for (int attempt = 0; attempt < 4; ++attempt) {  // a 64-bit hash collision between two words (only ever seen under COLIBRI_TEXT_HASH_BITS) is detected and retried with another seed
        DevState st{};
        st.cap = t.cap;
        HIP_TRY(c, hipMemcpyAsync(t.state.p, &st, sizeof st, hipMemcpyHostToDevice, c->stream));
        TextInfo reset = t.hinfo;
        reset.collision = reset.ndistinct = 0;
        HIP_TRY(c, hipMemcpyAsync(t.info.p, &reset, sizeof reset, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemsetAsync(t.first.p, 0xFF, sizeof(uint32_t) * t.cap, c->stream));
        hipLaunchKernelGGL(clear_table_kernel, dim3(stream_grid(t.cap)), dim3(kBlock), 0, c->stream, t.table.p, t.state.p);
        if (t.nevents) {
            const KeyWord fn{t.text.p, t.n, t.events.p, rules, 0x5851F42D4C957F2Dull * (uint64_t)(attempt + 1), retry_hash_mask("COLIBRI_TEXT_HASH_BITS", attempt)};
            Prof          p(c, COLIBRI_K_COUNT);
            hipLaunchKernelGGL((count_kernel<KeyWord>), dim3(std::max<uint32_t>(1, std::min<uint32_t>(blocks_for(t.nevents, kCountTile), 256u * 3u))), dim3(kBlock), 0, c->stream, fn,
                               t.slot_of.p, t.table.p, t.state.p, t.nevents, 1);
            hipLaunchKernelGGL(text_verify_kernel, dim3(stream_grid(t.nevents)), dim3(kBlock), 0, c->stream, t.text.p, t.n, t.events.p, t.nevents, rules, t.slot_of.p, t.table.p, t.first.p,
                               t.info.p);
            hipLaunchKernelGGL(text_words_kernel, dim3(stream_grid(t.cap)), dim3(kBlock), 0, c->stream, t.text.p, t.n, rules, t.events.p, t.table.p, t.cap, t.first.p, t.widx.p, t.wstart.p,
                               t.wlen.p, t.wcount.p, t.info.p);
        }
        TextInfo got{};
        HIP_TRY(c, hipMemcpyAsync(&got, t.info.p, sizeof got, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(&st, t.state.p, sizeof st, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        HIP_TRY(c, hipGetLastError());
        collect_events(c);  // (every attempt is one launch of COLIBRI_K_COUNT to colibri_kernel_time)
        if (st.overflow) return fail(c, COLIBRI_ERR_OVERFLOW, "word table exhausted");
        if (got.collision) continue;
        t.ndistinct = got.ndistinct;
        t.nwords    = st.admitted;
        t.rules     = rules;
        t.encoded   = false;
        *nwords     = t.nwords;
        *ndistinct  = t.ndistinct;
        return COLIBRI_OK;
    }
    return fail(c, COLIBRI_ERR_HIP, "word hashes collided under four different seeds");
}

int colibri_text_words(colibri_ctx* c, uint32_t* first_start, uint32_t* length, uint32_t* count) {
    if (!c) return COLIBRI_ERR_ARG;
    auto& t = c->tx;
    if (t.rules < 0) return fail(c, COLIBRI_ERR_STATE, "colibri_text_count first");
    HIP_TRY(c, hipSetDevice(c->device));
    if (t.ndistinct) {
        if (!first_start || !length || !count) return COLIBRI_ERR_ARG;
        HIP_TRY(c, hipMemcpy(first_start, t.wstart.p, sizeof(uint32_t) * t.ndistinct, hipMemcpyDeviceToHost));
        HIP_TRY(c, hipMemcpy(length, t.wlen.p, sizeof(uint32_t) * t.ndistinct, hipMemcpyDeviceToHost));
        HIP_TRY(c, hipMemcpy(count, t.wcount.p, sizeof(uint32_t) * t.ndistinct, hipMemcpyDeviceToHost));
    }
    return COLIBRI_OK;
}

int colibri_text_encode(colibri_ctx* c, const uint32_t* cls, const uint32_t* repeat, uint64_t* outbytes, uint64_t* ntokens, uint64_t* nlines) {
    if (!c || !outbytes || !ntokens || !nlines) return COLIBRI_ERR_ARG;
    auto& t = c->tx;
    if (t.rules != 1) return fail(c, COLIBRI_ERR_STATE, "colibri_text_count with the encoder's rules (1) first");
    if (t.ndistinct && (!cls || !repeat)) return COLIBRI_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    int            rc;
    const uint32_t nb = std::max<uint32_t>(1, blocks_for(t.nevents, kBlock * 4));
    if ((rc = dev_alloc(c, t.cls, (size_t)t.ndistinct + 1)) || (rc = dev_alloc(c, t.repeat, (size_t)t.ndistinct + 1)) || (rc = dev_alloc(c, t.outlen, (size_t)t.nevents + 1)) ||
        (rc = dev_alloc(c, t.outoff, (size_t)t.nevents + 1)) || (rc = dev_alloc(c, t.bsum, (size_t)nb + 1)))
        return rc;
    if (t.ndistinct) {
        HIP_TRY(c, hipMemcpyAsync(t.cls.p, cls, sizeof(uint32_t) * t.ndistinct, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(t.repeat.p, repeat, sizeof(uint32_t) * t.ndistinct, hipMemcpyHostToDevice, c->stream));
    }
    HIP_TRY(c, hipMemsetAsync(t.ntok.p, 0, sizeof(unsigned long long), c->stream));
    unsigned long long total = 0, ntok = 0;
    if (t.nevents) {
        Prof p(c, COLIBRI_K_EXPORT);
        hipLaunchKernelGGL(text_outlen_kernel, dim3(stream_grid(t.nevents)), dim3(kBlock), 0, c->stream, t.text.p, t.events.p, t.nevents, t.slot_of.p, t.widx.p, t.cls.p, t.repeat.p,
                           t.hinfo.after_last_nl, t.outlen.p, t.ntok.p);
        hipLaunchKernelGGL(scan_reduce_kernel, dim3(nb), dim3(kBlock), 0, c->stream, t.outlen.p, t.nevents, t.bsum.p);
        hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(kBlock), 0, c->stream, t.bsum.p, nb, t.bsum.p + nb);
        hipLaunchKernelGGL(scan_apply_kernel, dim3(nb), dim3(kBlock), 0, c->stream, t.outlen.p, t.nevents, t.bsum.p, t.outoff.p);
        HIP_TRY(c, hipMemcpyAsync(&total, t.bsum.p + nb, sizeof total, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(&ntok, t.ntok.p, sizeof ntok, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        if ((rc = dev_alloc(c, t.out, (size_t)total + 16))) return rc;
        hipLaunchKernelGGL(text_write_kernel, dim3(stream_grid(t.nevents)), dim3(kBlock), 0, c->stream, t.slot_of.p, t.nevents, t.widx.p, t.cls.p, t.repeat.p, t.outlen.p, t.outoff.p,
                           t.out.p);
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        HIP_TRY(c, hipGetLastError());
    } else if ((rc = dev_alloc(c, t.out, 16))) {
        return rc;
    }
    t.outbytes = total;
    t.encoded  = true;
    *outbytes  = total;
    *ntokens   = ntok;
    *nlines    = t.hinfo.nlines;
    return COLIBRI_OK;
}

int colibri_text_fetch(colibri_ctx* c, uint8_t* out) {
    if (!c) return COLIBRI_ERR_ARG;
    if (!c->tx.encoded) return fail(c, COLIBRI_ERR_STATE, "colibri_text_encode first");
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->tx.outbytes) {
        if (!out) return COLIBRI_ERR_ARG;
        HIP_TRY(c, hipMemcpy(out, c->tx.out.p, c->tx.outbytes, hipMemcpyDeviceToHost));
    }
    return COLIBRI_OK;
}

int colibri_text_as_corpus(colibri_ctx* c, uint32_t first_sentence) {
    if (!c) return COLIBRI_ERR_ARG;
    if (!c->tx.encoded) return fail(c, COLIBRI_ERR_STATE, "colibri_text_encode first");
    return colibri_upload_corpus_device(c, c->tx.out.p, c->tx.outbytes, first_sentence);
}

