// rindex_api.inc — part of colibri_hip.hip (included there, inside its extern "C" block, after print_api.inc): the reverse index of a pattern
// model over the uploaded corpus (colibri-patternmodeller -Z; kernels and the specification in rindex.hpp). The look-ups are the reverse-index
// stage of cooc_api.inc (rev_layers / rev_table / rev_probe), run over position ranges.

// the device pipeline on a model's keys in HBM, np == 0 included (V.cnt == NULL: only with occ == 0); the references are not read
static int rindex_core(colibri_ctx* c, const ModelView& V, uint32_t occ, int category, uint32_t size, uint64_t* npositions, uint64_t* nrows) {
    const uint32_t np       = V.np;
    const uint64_t keybytes = V.keybytes;
    auto&          ri = c->ri;
    int            rc;
    DevScratch     S{c};
    const uint64_t budget = env_u64("COLIBRI_RINDEX_BUDGET", kRindexBudgetBytes);
    const uint32_t npos = c->npos, ndelim = c->ndelim, nreal = npos - ndelim;  // (every delimiter is one position)
    DevBuf<uint8_t>            ntok;
    DevBuf<uint32_t>           pmask, info, memb, gate, hits, order, bad;
    DevBuf<unsigned long long> boff;
    DevBuf<CSlot>              table;
    // the layers the filters leave: category and size are per layer, so a layer that cannot pass is not looked up at all
    std::vector<std::pair<int, uint32_t>> layers;
    if (np) {
        if ((rc = S.take(ntok, np)) || (rc = S.take(pmask, np)) || (rc = S.take(info, 4))) return rc;
        const uint32_t info0[4] = {0xFFFFFFFFu, 0u, 0u, 0u};
        HIP_TRY(c, hipMemcpyAsync(info.p, info0, sizeof info0, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(cooc_info_kernel, dim3(stream_grid(np)), dim3(kBlock), 0, c->stream, V.kbytes, V.koff, np, ntok.p, pmask.p, info.p);
        RevLayers RL;
        if ((rc = rev_layers(c, "rindex", COLIBRI_ERR_OVERFLOW, ntok.p, pmask.p, info.p, np, RL))) return rc;
        for (const auto& l : RL.layers) {
            if (size != 0 && (uint32_t)l.first != size) continue;
            if (l.second == 0 ? (category == 0 || category == 1) : (category == 0 || category == 2)) layers.push_back(l);
        }
        S.drop(ntok);
        S.drop(pmask);
        S.drop(info);
    }
    const uint32_t        L = (uint32_t)layers.size();
    std::vector<uint32_t> horder(L);
    for (uint32_t l = 0; l < L; ++l) horder[l] = l;
    std::sort(horder.begin(), horder.end(), [&](uint32_t a, uint32_t b) { return layers[a] < layers[b]; });  // by n, the n-gram (mask 0) first, masks ascending
    // position-range chunks: the layer array costs 4 bytes x layers x positions
    const uint64_t cap64   = 2ull * np + 1024;
    const uint64_t per_pos = 4ull * L + 4 + 4 + 8;  // memb, gate, hits, boff
    const uint64_t fixed   = sizeof(CSlot) * cap64 + 14ull * ((uint64_t)nreal + 1) + 8 + keybytes + 16 + 8ull * ((uint64_t)np + 1) + 4ull * L + 64;
    if (fixed > budget)
        return fail(c, COLIBRI_ERR_OVERFLOW, "rindex: %u patterns and %u positions need %llu bytes, above the budget of %llu bytes (COLIBRI_RINDEX_BUDGET)", np, nreal,
                    (unsigned long long)fixed, (unsigned long long)budget);
    uint64_t chunk = env_u64("COLIBRI_RINDEX_CHUNK", 0);  // (tests: many small chunks on a small corpus)
    if (chunk == 0) chunk = (budget - fixed) / 2 / per_pos;
    chunk = std::min<uint64_t>(chunk, std::max<uint32_t>(npos, 1u));
    if (chunk == 0 || fixed + (chunk + 1) * per_pos > budget)
        return fail(c, COLIBRI_ERR_OVERFLOW, "rindex: %u layers over a chunk of positions need %llu bytes per position beside %llu bytes, above the budget of %llu bytes (COLIBRI_RINDEX_BUDGET)",
                    L, (unsigned long long)per_pos, (unsigned long long)fixed, (unsigned long long)budget);
    const uint32_t C       = (uint32_t)chunk;
    const uint64_t nchunks = ((uint64_t)npos + C - 1) / C;
    const size_t   stride  = (size_t)C + 1;
    const uint32_t cap     = (uint32_t)cap64;
    if ((rc = dev_alloc(c, ri.pos_off, (size_t)nreal + 1)) || (rc = dev_alloc(c, ri.sentence, (size_t)nreal + 1)) || (rc = dev_alloc(c, ri.token, (size_t)nreal + 1))) return rc;
    if ((rc = S.take(table, (size_t)cap64)) || (rc = S.take(memb, (size_t)L * stride)) || (rc = S.take(gate, stride)) || (rc = S.take(hits, stride)) || (rc = S.take(boff, stride)) ||
        (rc = S.take(order, L)) || (rc = S.take(bad, 1)))
        return rc;
    HIP_TRY(c, hipMemsetAsync(bad.p, 0, sizeof(uint32_t), c->stream));
    if (L) HIP_TRY(c, hipMemcpyAsync(order.p, horder.data(), sizeof(uint32_t) * L, hipMemcpyHostToDevice, c->stream));
    {
        Prof p(c, COLIBRI_K_COUNT);
        if ((rc = rev_table(c, V.kbytes, V.koff, np, table.p, cap))) return rc;
    }
    unsigned long long base = 0;
    uint64_t           pcap = ri.pattern.p ? ri.pattern.n : 0;
    for (uint64_t j = 0; j < nchunks; ++j) {
        const uint32_t p0 = (uint32_t)(j * C), n = std::min<uint32_t>(C, npos - p0);
        {
            Prof p(c, COLIBRI_K_COUNT);
            rev_probe(c, V.kbytes, V.koff, layers, table.p, cap, p0, n, memb.p, stride, gate.p);
        }
        unsigned long long EB = 0;
        hipLaunchKernelGGL(rindex_hits_kernel, dim3(stream_grid((uint64_t)n + 1)), dim3(kBlock), 0, c->stream, memb.p, stride, L, n, V.cnt, occ, hits.p);
        if ((rc = scan_u32(c, hits.p, n + 1, boff.p, &EB))) return rc;
        if (EB >= 0xFFFFFFF0ull || base + EB >= 0xFFFFFFF0ull)
            return fail(c, COLIBRI_ERR_OVERFLOW, "rindex: %llu rows (at most 2^32 - 16)", (unsigned long long)(base + EB));
        if (base + EB + 1 > pcap) {  // the rows so far: grow, keeping what they hold
            const uint64_t want = std::max<uint64_t>(base + EB + 1, pcap + pcap / 2);
            if (fixed + (chunk + 1) * per_pos + 4 * want + (base ? 4 * pcap : 0) > budget)
                return fail(c, COLIBRI_ERR_OVERFLOW, "rindex: %llu rows beside %llu bytes of scratch exceed the budget of %llu bytes (COLIBRI_RINDEX_BUDGET)",
                            (unsigned long long)(base + EB), (unsigned long long)(fixed + (chunk + 1) * per_pos), (unsigned long long)budget);
            DevBuf<uint32_t> grown;
            if (base == 0) ri.pattern.reset();
            if ((rc = dev_alloc(c, grown, (size_t)want))) return rc;
            if (base) HIP_TRY(c, hipMemcpyAsync(grown.p, ri.pattern.p, sizeof(uint32_t) * base, hipMemcpyDeviceToDevice, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));  // (the old buffer goes)
            ri.pattern = std::move(grown);
            pcap       = want;
        }
        hipLaunchKernelGGL(rindex_fill_kernel, dim3(stream_grid(n)), dim3(kBlock), 0, c->stream, memb.p, stride, L, order.p, p0, n, c->cs.rem.p, c->delimpos.p, ndelim, c->first_sentence,
                           V.cnt, occ, boff.p, base, ri.pos_off.p, ri.sentence.p, ri.token.p, ri.pattern.p, bad.p);
        base += EB;
    }
    if (!ri.pattern.p && (rc = dev_alloc(c, ri.pattern, 1))) return rc;
    uint32_t hbad = 0;
    HIP_TRY(c, hipMemcpyAsync(ri.pos_off.p + nreal, &base, sizeof base, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(&hbad, bad.p, sizeof hbad, hipMemcpyDeviceToHost, c->stream));
    // the model's keys stay with the index: the text is written from them
    if ((rc = dev_alloc(c, ri.kbytes, (size_t)keybytes + 16)) || (rc = dev_alloc(c, ri.koff, (size_t)np + 1))) return rc;
    if (np) {
        HIP_TRY(c, hipMemcpyAsync(ri.kbytes.p, V.kbytes, keybytes + 16, hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(ri.koff.p, V.koff, sizeof(unsigned long long) * ((size_t)np + 1), hipMemcpyDeviceToDevice, c->stream));
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    collect_events(c);
    if (hbad & kRindexBadToken) return fail(c, COLIBRI_ERR_OVERFLOW, "rindex: a sentence of more than 65536 tokens (token indices are 16-bit)");
    ri.np         = np;
    ri.npositions = nreal;
    ri.nrows      = base;
    ri.chunks     = nchunks;
    ri.scratch    = S.peak;
    ri.valid      = true;
    *npositions   = nreal;
    *nrows        = base;
    return COLIBRI_OK;
}

static int rindex_begin(colibri_ctx* c, int category, uint64_t size, uint64_t* npositions, uint64_t* nrows) {
    if (!c || !npositions || !nrows || category < 0 || category > 3 || size > 0xFFFFFFFFull) return COLIBRI_ERR_ARG;
    auto& ri = c->ri;
    ri.valid = false;
    ri.npositions = ri.nrows = ri.chunks = ri.windows = ri.staging = ri.scratch = 0;
    *npositions = *nrows = 0;
    if (!c->have_corpus) return fail(c, COLIBRI_ERR_STATE, "rindex needs the corpus uploaded (colibri_upload_corpus): it is the reverse index");
    if (c->sh.active) return fail(c, COLIBRI_ERR_STATE, "rindex: the context holds a sharded run (a part of the corpus)");
    return COLIBRI_OK;
}

int colibri_rindex(colibri_ctx* c, const uint64_t* key_off, const uint8_t* key_bytes, const uint32_t* counts, uint64_t npatterns, uint32_t occurrencecount, int category, uint64_t size,
                   uint64_t* npositions, uint64_t* nrows) {
    int rc = rindex_begin(c, category, size, npositions, nrows);
    if (rc) return rc;
    if (occurrencecount && npatterns && !counts) return fail(c, COLIBRI_ERR_ARG, "rindex: an occurrence threshold needs the patterns' counts");
    ModelView V;
    if ((rc = model_upload(c, "rindex", key_off, key_bytes, counts, nullptr, nullptr, nullptr, npatterns, kModelCounts, V))) return rc;
    return rindex_core(c, V, occurrencecount, category, (uint32_t)size, npositions, nrows);
}

// the same on the model of the last colibri_train of this context, indexed or not, where it lies in HBM with its corpus
int colibri_rindex_resident(colibri_ctx* c, uint32_t occurrencecount, int category, uint64_t size, uint64_t* npositions, uint64_t* nrows) {
    int rc = rindex_begin(c, category, size, npositions, nrows);
    if (rc) return rc;
    ModelView V;
    if ((rc = model_resident(c, "colibri_rindex_resident", false, V))) return rc;
    // a trained model of no patterns still has an index, of empty rows: the empty model's buffers
    if (V.np == 0 && (rc = model_upload(c, "rindex", nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, V))) return rc;
    return rindex_core(c, V, occurrencecount, category, (uint32_t)size, npositions, nrows);
}

int colibri_rindex_fetch(colibri_ctx* c, uint64_t* pos_off, uint32_t* sentence, uint16_t* token, uint32_t* pattern) {
    if (!c) return COLIBRI_ERR_ARG;
    auto& ri = c->ri;
    if (!ri.valid) return fail(c, COLIBRI_ERR_STATE, "colibri_rindex / colibri_rindex_resident first");
    HIP_TRY(c, hipSetDevice(c->device));
    const uint64_t P = ri.npositions, K = ri.nrows;
    if (pos_off) HIP_TRY(c, hipMemcpyAsync(pos_off, ri.pos_off.p, sizeof(uint64_t) * (P + 1), hipMemcpyDeviceToHost, c->stream));
    if (sentence && P) HIP_TRY(c, hipMemcpyAsync(sentence, ri.sentence.p, sizeof(uint32_t) * P, hipMemcpyDeviceToHost, c->stream));
    if (token && P) HIP_TRY(c, hipMemcpyAsync(token, ri.token.p, sizeof(uint16_t) * P, hipMemcpyDeviceToHost, c->stream));
    if (pattern && K) HIP_TRY(c, hipMemcpyAsync(pattern, ri.pattern.p, sizeof(uint32_t) * K, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return COLIBRI_OK;
}

// printreverseindex's text of the last index, through output windows and the decoder's pinned double buffers, as print_core hands its windows over
int colibri_rindex_text(colibri_ctx* c, colibri_decode_sink sink, void* user, uint64_t* outbytes) {
    if (!c || !sink) return COLIBRI_ERR_ARG;
    auto& ri = c->ri;
    auto& d  = c->dc;
    if (outbytes) *outbytes = 0;
    ri.windows = ri.staging = 0;
    if (!ri.valid) return fail(c, COLIBRI_ERR_STATE, "colibri_rindex_text: colibri_rindex / colibri_rindex_resident first");
    if (!c->pr.table) return fail(c, COLIBRI_ERR_STATE, "colibri_rindex_text: no word table installed by colibri_print_classes");
    HIP_TRY(c, hipSetDevice(c->device));
    int            rc;
    DevScratch     S{c};
    const uint64_t budget = env_u64("COLIBRI_RINDEX_BUDGET", kRindexBudgetBytes);
    const uint32_t np = ri.np, nreal = (uint32_t)ri.npositions;
    DevBuf<uint32_t>           tlen, linelen, bad;
    DevBuf<unsigned long long> toff, linestart, range;
    DevBuf<uint8_t>            arena;
    const PrintTable           tab{c->pr.wordoff.p, c->pr.words.p, c->pr.has.p, c->pr.nids};
    // (a) the pattern-text arena
    unsigned long long textbytes = 0, total = 0;
    if ((rc = S.take(tlen, (size_t)np + 1)) || (rc = S.take(toff, (size_t)np + 1)) || (rc = S.take(bad, 1))) return rc;
    HIP_TRY(c, hipMemsetAsync(bad.p, 0, sizeof(uint32_t), c->stream));
    hipLaunchKernelGGL(rindex_textlen_kernel, dim3(stream_grid((uint64_t)np + 1)), dim3(kBlock), 0, c->stream, ri.kbytes.p, ri.koff.p, np, tab, tlen.p, bad.p);
    if ((rc = scan_u32(c, tlen.p, np + 1, toff.p, &textbytes))) return rc;
    const uint64_t need = 12ull * ((uint64_t)np + 1) + textbytes + 12ull * ((uint64_t)nreal + 2) + 64;
    if (need > budget)
        return fail(c, COLIBRI_ERR_OVERFLOW, "rindex text: %u patterns and %u positions need %llu bytes of scratch, above the budget of %llu bytes (COLIBRI_RINDEX_BUDGET)", np, nreal,
                    (unsigned long long)need, (unsigned long long)budget);
    if ((rc = S.take(arena, (size_t)textbytes + 1)) || (rc = S.take(linelen, (size_t)nreal + 2)) || (rc = S.take(linestart, (size_t)nreal + 2)) || (rc = S.take(range, 4))) return rc;
    hipLaunchKernelGGL(rindex_arena_kernel, dim3(stream_grid(np)), dim3(kBlock), 0, c->stream, ri.kbytes.p, ri.koff.p, np, tab, toff.p, arena.p);
    // (b) the lines' lengths and their scan
    hipLaunchKernelGGL(rindex_linelen_kernel, dim3(stream_grid((uint64_t)nreal + 2)), dim3(kBlock), 0, c->stream, ri.pos_off.p, ri.sentence.p, ri.token.p, ri.pattern.p, tlen.p, nreal,
                       linelen.p, bad.p);
    if ((rc = scan_u32(c, linelen.p, nreal + 2, linestart.p, &total))) return rc;
    uint32_t hbad = 0;
    HIP_TRY(c, hipMemcpy(&hbad, bad.p, sizeof hbad, hipMemcpyDeviceToHost));
    if (hbad & kRindexBadLine) return fail(c, COLIBRI_ERR_OVERFLOW, "rindex text: a line of 4 GiB or more");
    S.drop(linelen);
    // (c) windows of B bytes: the device writes window w into stage[w & 1] and copies it to pinned[w & 1] while the host hands window w - 1 to the sink
    const uint64_t B = std::min<uint64_t>(env_u64("COLIBRI_RINDEX_WINDOW_BYTES", kRindexWindowBytes), total);
    if (need + 2 * B > budget)
        return fail(c, COLIBRI_ERR_OVERFLOW, "rindex text: two windows of %llu bytes beside %llu bytes of scratch exceed the budget of %llu bytes (COLIBRI_RINDEX_BUDGET)",
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
    ri.scratch        = std::max<uint64_t>(ri.scratch, S.peak);
    const uint64_t nw = (total + B - 1) / B;
    auto hand_over = [&](uint64_t w) -> int {
        HIP_TRY(c, hipEventSynchronize(d.ev[w & 1]));
        const uint64_t n = std::min<uint64_t>(B, total - w * B);
        if (const int s = sink(user, d.pinned[w & 1], n))
            return fail(c, COLIBRI_ERR_STATE, "rindex text: the sink stopped the call (it returned %d) after %llu bytes", s, (unsigned long long)(w * B));
        return COLIBRI_OK;
    };
    const uint32_t grid = stream_grid(std::min<uint64_t>(std::max<uint64_t>(ri.nrows, (uint64_t)nreal + 1), B + 1));  // (a window of B bytes holds fewer than B lines or entries, but for its two cut lines)
    for (uint64_t w = 0; w < nw; ++w) {
        const unsigned long long W0 = w * B, W1 = std::min<uint64_t>(total, W0 + B);
        hipLaunchKernelGGL(rindex_range_kernel, dim3(1), dim3(kWave), 0, c->stream, linestart.p, ri.pos_off.p, nreal, W0, W1, range.p);
        hipLaunchKernelGGL(rindex_head_kernel, dim3(grid), dim3(kBlock), 0, c->stream, linestart.p, ri.sentence.p, ri.token.p, nreal, range.p, W0, W1, stage[w & 1].p);
        if (ri.nrows)
            hipLaunchKernelGGL(rindex_entry_kernel, dim3(grid), dim3(kBlock), 0, c->stream, linestart.p, ri.pos_off.p, ri.sentence.p, ri.token.p, ri.pattern.p, tlen.p, toff.p, arena.p,
                               nreal, range.p, W0, W1, stage[w & 1].p);
        HIP_TRY(c, hipMemcpyAsync(d.pinned[w & 1], stage[w & 1].p, W1 - W0, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipEventRecord(d.ev[w & 1], c->stream));
        if (w > 0 && (rc = hand_over(w - 1))) {
            (void)hipStreamSynchronize(c->stream);
            return rc;
        }
    }
    if ((rc = hand_over(nw - 1))) return rc;
    HIP_TRY(c, hipGetLastError());
    ri.windows = nw;
    ri.staging = 2 * B;
    if (outbytes) *outbytes = total;
    return COLIBRI_OK;
}

int colibri_rindex_info(const colibri_ctx* c, uint64_t* chunks, uint64_t* windows, uint64_t* staging_bytes, uint64_t* scratch_bytes) {
    if (!c) return COLIBRI_ERR_ARG;
    if (chunks) *chunks = c->ri.chunks;
    if (windows) *windows = c->ri.windows;
    if (staging_bytes) *staging_bytes = c->ri.staging;
    if (scratch_bytes) *scratch_bytes = c->ri.scratch;
    return COLIBRI_OK;
}
