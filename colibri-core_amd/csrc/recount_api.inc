// recount_api.inc — part of colibri_hip.hip (included there, inside its extern "C" block, after subsume_api.inc): the skipgrams of an in-place
// rebuild, counted on the uploaded corpus (colibri-patternmodeller -I -s; kernels and the specification in recount.hpp). The key table and the
// masked probes are the reverse-index stage of cooc_api.inc (rev_table / rev_probe), run over position ranges.

// the device pipeline on skipgram keys in HBM, np == 0 included
static int recount_core(colibri_ctx* c, const ModelView& V, bool indexed, uint32_t mintokens, uint64_t* nkept, uint64_t* nrefs) {
    auto&          rk = c->rk;
    const uint32_t np = V.np;
    int            rc;
    DevScratch     S{c};
    rk.np      = np;
    rk.indexed = indexed;
    if ((rc = dev_alloc(c, rk.counts, np)) || (rc = dev_alloc(c, rk.ref_off, (size_t)np + 1))) return rc;
    HIP_TRY(c, hipMemsetAsync(rk.counts.p, 0, sizeof(uint32_t) * std::max<size_t>(np, 1), c->stream));
    HIP_TRY(c, hipMemsetAsync(rk.ref_off.p, 0, sizeof(unsigned long long) * ((size_t)np + 1), c->stream));
    if (np == 0) {
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        rk.valid = true;
        return COLIBRI_OK;
    }
    for (size_t len = 65536; len < c->lenhist.size(); ++len)
        if (c->lenhist[len]) return fail(c, COLIBRI_ERR_UNSUPPORTED, "recount: a sentence of 65536 tokens or more (token indices are 16-bit)");
    const uint64_t budget = env_u64("COLIBRI_RECOUNT_BUDGET", kRindexBudgetBytes);
    const uint32_t npos = c->npos, ndelim = c->ndelim;
    DevBuf<uint8_t>            ntok;
    DevBuf<uint32_t>           pmask, info, memb, gate, hits, kept, done, small, key[2], val[2];
    DevBuf<unsigned long long> boff;
    DevBuf<CSlot>              table;
    // the keys' groups: every key has to be a skipgram of 3 .. kMaskedMaxTokens tokens
    if ((rc = S.take(ntok, np)) || (rc = S.take(pmask, np)) || (rc = S.take(info, 4))) return rc;
    const uint32_t info0[4] = {0xFFFFFFFFu, 0u, 0u, 0u};
    HIP_TRY(c, hipMemcpyAsync(info.p, info0, sizeof info0, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(cooc_info_kernel, dim3(stream_grid(np)), dim3(kBlock), 0, c->stream, V.kbytes, V.koff, np, ntok.p, pmask.p, info.p);
    uint32_t              hinfo[4];
    std::vector<uint8_t>  hn(np);
    std::vector<uint32_t> hm(np);
    HIP_TRY(c, hipMemcpyAsync(hinfo, info.p, sizeof hinfo, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(hn.data(), ntok.p, np, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(hm.data(), pmask.p, sizeof(uint32_t) * np, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    S.drop(ntok);
    S.drop(pmask);
    S.drop(info);
    if (hinfo[3] & 4u) return fail(c, COLIBRI_ERR_UNSUPPORTED, "recount: a key is a flexgram (the reference matches them by flexgramsize, outside this build)");
    std::vector<std::pair<int, uint32_t>> layers;
    for (uint32_t p = 0; p < np; ++p) {
        if (hm[p] == 0 || hn[p] < 3) return fail(c, COLIBRI_ERR_UNSUPPORTED, "recount: key %u is not a skipgram of three or more tokens", p);
        if (hn[p] > kMaskedMaxTokens) return fail(c, COLIBRI_ERR_UNSUPPORTED, "recount: skipgrams of more than %d tokens", kMaskedMaxTokens);
        layers.push_back({(int)hn[p], hm[p]});
    }
    std::sort(layers.begin(), layers.end());
    layers.erase(std::unique(layers.begin(), layers.end()), layers.end());
    const uint32_t L = (uint32_t)layers.size();
    // position-range chunks: the group array costs 4 bytes x groups x positions
    const uint64_t cap64 = 2ull * np + 1024;
    if (cap64 >= 0xFFFFFFF0ull) return fail(c, COLIBRI_ERR_OVERFLOW, "recount: %u keys exceed the key table's 32-bit slots", np);
    const uint64_t per_pos = 4ull * L + 4 + 4 + 8;  // memb, gate, hits, boff
    const uint64_t fixed   = sizeof(CSlot) * cap64 + V.keybytes + 16 + 8ull * ((uint64_t)np + 1) + 20ull * ((uint64_t)np + 1) + 64;  // table, keys, counts / kept / done / ref_off
    if (fixed > budget)
        return fail(c, COLIBRI_ERR_OVERFLOW, "recount: %u keys need %llu bytes, above the budget of %llu bytes (COLIBRI_RECOUNT_BUDGET)", np, (unsigned long long)fixed,
                    (unsigned long long)budget);
    uint64_t chunk = env_u64("COLIBRI_RECOUNT_CHUNK", 0);  // (tests: many small chunks on a small corpus)
    if (chunk == 0) chunk = (budget - fixed) / 2 / per_pos;
    chunk = std::min<uint64_t>(chunk, std::max<uint32_t>(npos, 1u));
    if (chunk == 0 || fixed + (chunk + 1) * per_pos > budget)
        return fail(c, COLIBRI_ERR_OVERFLOW, "recount: %u groups over a chunk of positions need %llu bytes per position beside %llu bytes, above the budget of %llu bytes (COLIBRI_RECOUNT_BUDGET)",
                    L, (unsigned long long)per_pos, (unsigned long long)fixed, (unsigned long long)budget);
    const uint32_t C       = (uint32_t)chunk;
    const uint64_t nchunks = ((uint64_t)npos + C - 1) / C;
    const size_t   stride  = (size_t)C + 1;
    const uint32_t cap     = (uint32_t)cap64;
    if ((rc = S.take(table, (size_t)cap64)) || (rc = S.take(memb, (size_t)L * stride)) || (rc = S.take(gate, stride)) || (rc = S.take(kept, (size_t)np + 1)) || (rc = S.take(small, 1)))
        return rc;
    HIP_TRY(c, hipMemsetAsync(small.p, 0, sizeof(uint32_t), c->stream));
    {
        Prof p(c, COLIBRI_K_COUNT);
        if ((rc = rev_table(c, V.kbytes, V.koff, np, table.p, cap))) return rc;
        // pass 1: the counts
        for (uint64_t j = 0; j < nchunks; ++j) {
            const uint32_t p0 = (uint32_t)(j * C), n = std::min<uint32_t>(C, npos - p0);
            rev_probe(c, V.kbytes, V.koff, layers, table.p, cap, p0, n, memb.p, stride, gate.p);
            hipLaunchKernelGGL(recount_count_kernel, dim3(stream_grid(n)), dim3(kBlock), 0, c->stream, memb.p, stride, L, n, rk.counts.p);
        }
    }
    unsigned long long R = 0;
    uint32_t           K = 0;
    hipLaunchKernelGGL(recount_kept_kernel, dim3(stream_grid((uint64_t)np + 1)), dim3(kBlock), 0, c->stream, rk.counts.p, np, mintokens, kept.p, small.p);
    if ((rc = scan_u32(c, kept.p, np + 1, rk.ref_off.p, &R))) return rc;  // (waits)
    HIP_TRY(c, hipMemcpy(&K, small.p, sizeof K, hipMemcpyDeviceToHost));
    if (R >= 0xFFFFFFF0ull) return fail(c, COLIBRI_ERR_OVERFLOW, "recount: %llu references (at most 2^32 - 16)", R);
    if (indexed) {
        const uint64_t held = fixed + (chunk + 1) * per_pos + 6ull * (R + 1);
        if (held > budget)
            return fail(c, COLIBRI_ERR_OVERFLOW, "recount: %llu references beside %llu bytes of scratch exceed the budget of %llu bytes (COLIBRI_RECOUNT_BUDGET)", R,
                        (unsigned long long)(fixed + (chunk + 1) * per_pos), (unsigned long long)budget);
        if ((rc = dev_alloc(c, rk.ref_sentence, (size_t)R + 1)) || (rc = dev_alloc(c, rk.ref_token, (size_t)R + 1))) return rc;
        if ((rc = S.take(hits, stride)) || (rc = S.take(boff, stride)) || (rc = S.take(done, np))) return rc;
        HIP_TRY(c, hipMemsetAsync(done.p, 0, sizeof(uint32_t) * np, c->stream));
        const int bits = bits_for(np);
        // pass 2: the references, chunk after chunk
        for (uint64_t j = 0; j < nchunks && R; ++j) {
            const uint32_t p0 = (uint32_t)(j * C), n = std::min<uint32_t>(C, npos - p0);
            {
                Prof p(c, COLIBRI_K_COUNT);
                rev_probe(c, V.kbytes, V.koff, layers, table.p, cap, p0, n, memb.p, stride, gate.p);
            }
            unsigned long long EB = 0;
            hipLaunchKernelGGL(rindex_hits_kernel, dim3(stream_grid((uint64_t)n + 1)), dim3(kBlock), 0, c->stream, memb.p, stride, L, n, rk.counts.p, mintokens, hits.p);
            if ((rc = scan_u32(c, hits.p, n + 1, boff.p, &EB))) return rc;
            if (EB == 0) continue;
            if (EB > R) return fail(c, COLIBRI_ERR_STATE, "recount: a chunk holds %llu hits of %llu counted", EB, R);
            if (!key[0].p || key[0].n < EB) {  // the chunk's pairs and their sort's other side: grown to the largest chunk
                if (held + 16ull * EB > budget)
                    return fail(c, COLIBRI_ERR_OVERFLOW, "recount: %llu hits in one chunk beside %llu bytes exceed the budget of %llu bytes (COLIBRI_RECOUNT_BUDGET)", EB,
                                (unsigned long long)held, (unsigned long long)budget);
                for (int b = 0; b < 2; ++b) {
                    S.drop(key[b]);
                    S.drop(val[b]);
                }
                for (int b = 0; b < 2; ++b)
                    if ((rc = S.take(key[b], (size_t)EB)) || (rc = S.take(val[b], (size_t)EB))) return rc;
            }
            Prof           p(c, COLIBRI_K_INDEX);
            const uint32_t m = (uint32_t)EB;
            hipLaunchKernelGGL(recount_pairs_kernel, dim3(stream_grid(n)), dim3(kBlock), 0, c->stream, memb.p, stride, L, p0, n, rk.counts.p, mintokens, boff.p, key[0].p, val[0].p);
            uint32_t* const keys[2] = {key[0].p, key[1].p};
            uint32_t* const vals[2] = {val[0].p, val[1].p};
            int             cur     = 0;
            if ((rc = radix_sort_pairs(c, keys, vals, m, bits, cur))) return rc;
            hipLaunchKernelGGL(recount_refs_kernel, dim3(stream_grid(m)), dim3(kBlock), 0, c->stream, keys[cur], vals[cur], m, rk.ref_off.p, done.p, c->delimpos.p, ndelim, c->first_sentence,
                               rk.ref_sentence.p, rk.ref_token.p);
            hipLaunchKernelGGL(recount_done_kernel, dim3(stream_grid(m)), dim3(kBlock), 0, c->stream, keys[cur], m, done.p);
        }
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    collect_events(c);
    rk.nrefs   = indexed ? R : 0;
    rk.nkept   = K;
    rk.groups  = L;
    rk.chunks  = nchunks;
    rk.scratch = S.peak;
    rk.valid   = true;
    *nkept     = K;
    *nrefs     = rk.nrefs;
    return COLIBRI_OK;
}

int colibri_recount(colibri_ctx* c, const uint64_t* key_off, const uint8_t* key_bytes, uint64_t npatterns, int indexed, uint32_t mintokens, uint64_t* nkept, uint64_t* nrefs) {
    if (!c || !nkept || !nrefs) return COLIBRI_ERR_ARG;
    auto& rk = c->rk;
    rk.valid = false;
    rk.np    = 0;
    rk.nrefs = rk.nkept = rk.groups = rk.chunks = rk.scratch = 0;
    *nkept = *nrefs = 0;
    if (!c->have_corpus) return fail(c, COLIBRI_ERR_STATE, "recount needs the corpus uploaded (colibri_upload_corpus): the skipgrams are counted on it");
    if (c->sh.active) return fail(c, COLIBRI_ERR_STATE, "recount: the context holds a sharded run (a part of the corpus)");
    ModelView V;
    int       rc;
    if ((rc = model_upload(c, "recount", key_off, key_bytes, nullptr, nullptr, nullptr, nullptr, npatterns, 0, V))) return rc;
    return recount_core(c, V, indexed != 0, std::max<uint32_t>(mintokens, 1u), nkept, nrefs);
}

// the arrays of the last call, aligned to its keys (any may be NULL): counts (npatterns), and of an indexed call ref_off (npatterns + 1) and the
// references (nrefs each)
int colibri_recount_fetch(colibri_ctx* c, uint32_t* counts, uint64_t* ref_off, uint32_t* ref_sentence, uint16_t* ref_token) {
    if (!c) return COLIBRI_ERR_ARG;
    auto& rk = c->rk;
    if (!rk.valid) return fail(c, COLIBRI_ERR_STATE, "colibri_recount first");
    HIP_TRY(c, hipSetDevice(c->device));
    const uint64_t P = rk.np, K = rk.nrefs;
    if (counts && P) HIP_TRY(c, hipMemcpyAsync(counts, rk.counts.p, sizeof(uint32_t) * P, hipMemcpyDeviceToHost, c->stream));
    if (ref_off && rk.indexed) HIP_TRY(c, hipMemcpyAsync(ref_off, rk.ref_off.p, sizeof(uint64_t) * (P + 1), hipMemcpyDeviceToHost, c->stream));
    if (ref_sentence && K) HIP_TRY(c, hipMemcpyAsync(ref_sentence, rk.ref_sentence.p, sizeof(uint32_t) * K, hipMemcpyDeviceToHost, c->stream));
    if (ref_token && K) HIP_TRY(c, hipMemcpyAsync(ref_token, rk.ref_token.p, sizeof(uint16_t) * K, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return COLIBRI_OK;
}

int colibri_recount_info(const colibri_ctx* c, uint64_t* groups, uint64_t* chunks, uint64_t* scratch_bytes) {
    if (!c) return COLIBRI_ERR_ARG;
    if (groups) *groups = c->rk.groups;
    if (chunks) *chunks = c->rk.chunks;
    if (scratch_bytes) *scratch_bytes = c->rk.scratch;
    return COLIBRI_OK;
}
