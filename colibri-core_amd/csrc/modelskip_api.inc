// modelskip_api.inc — part of colibri_hip.hip (included there, inside its extern "C" block, after recount_api.inc): the skipgrams of an indexed
// model that holds its n-grams already (IndexedPatternModel::trainskipgrams, colibri-patternmodeller -i model -s; kernels and the specification
// in modelskip.hpp, DESIGN.md §5m). No corpus is needed. The answer is the skipgrams (by order, then by group rank) and one keep byte per input
// pattern; the model itself, uploaded or resident, is only read.

// scan_u32 with its three kernels inside a bracket of class `cls` and the read of the total (a blocking copy) outside it, so that a profiled call's class
// times hold the scans and no idle stream (the total lies behind scan_u32's block sums)
static int mskip_scan(colibri_ctx* c, int cls, const uint32_t* in, uint32_t n, unsigned long long* out, unsigned long long* total) {
    int rc;
    {
        Prof prof(c, cls);
        if ((rc = scan_u32(c, in, n, out, nullptr))) return rc;
    }
    if (total) {
        const uint32_t nb = std::max<uint32_t>(1, blocks_for(n, kBlock * 4));
        HIP_TRY(c, hipMemcpyAsync(total, c->bsum.p + nb, sizeof *total, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        HIP_TRY(c, hipGetLastError());
    }
    return COLIBRI_OK;
}

// the device pipeline on an indexed model in HBM (np > 0)
static int mskip_core(colibri_ctx* c, const ModelView& V, uint32_t t, bool check, uint32_t mintypes, int maxlength, int maxskips) {
    auto&          ms = c->ms;
    const uint32_t np = V.np;
    int            rc;
    DevScratch     S{c};
    DevBuf<uint8_t>            ntok, live, mbytes;
    DevBuf<uint32_t>           pmask, words, flag, src, masks_d, clen, slot_of, isrep, gcnt, gtypes, grep, gkeep, kcnt, klen, contrib, iref, gref, key[2], val[2];
    DevBuf<unsigned long long> vrank, moff, rank, krank, kkoff, kroff, soff;
    DevBuf<CSlot>              table;
    DevBuf<MSlot>              gtable;
    DevBuf<MskipInfo>          info;
    if ((rc = S.take(ntok, np)) || (rc = S.take(live, np)) || (rc = S.take(pmask, np)) || (rc = S.take(words, 4)) || (rc = S.take(info, 1))) return rc;
    uint32_t hw[4] = {0xFFFFFFFFu, 0, 0, 0};
    HIP_TRY(c, hipMemcpyAsync(words.p, hw, sizeof hw, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(cooc_info_kernel, dim3(stream_grid(np)), dim3(kBlock), 0, c->stream, V.kbytes, V.koff, np, ntok.p, pmask.p, words.p);
    HIP_TRY(c, hipMemcpyAsync(hw, words.p, sizeof hw, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // the one look at the model ahead of the orders: its categories and its longest pattern
    HIP_TRY(c, hipGetLastError());
    S.drop(pmask);
    if (hw[3] & 6u)
        return fail(c, COLIBRI_ERR_UNSUPPORTED, "modelskip: the model already holds %s (their references would be added a second time); pass a model of n-grams only",
                    (hw[3] & 4u) ? "flexgrams" : "skipgrams");
    const uint32_t top = (uint32_t)std::min<int64_t>(maxlength, hw[1]);  // (above the longest pattern nothing is found)
    if (top > (uint32_t)kMskipMaxTokens)
        return fail(c, COLIBRI_ERR_UNSUPPORTED, "modelskip: a source n-gram of %u tokens (a gap mask holds %d)", top, kMskipMaxTokens);
    HIP_TRY(c, hipMemsetAsync(ms.keep.p, 1, np, c->stream));
    HIP_TRY(c, hipMemsetAsync(live.p, 1, np, c->stream));
    if (top < 3) {  // (order 3 was looked at and found nothing, as mskip_begin left it)
        ms.scratch = S.peak;
        return COLIBRI_OK;
    }
    const uint64_t cap64 = 2ull * np + 1024;
    if (cap64 >= 0xFFF00000ull)  // (constraint_clear_kernel counts its slots in 32 bits under a stride of up to 2^20)
        return fail(c, COLIBRI_ERR_OVERFLOW, "modelskip: %u patterns exceed the key table's 32-bit slots", np);
    const uint32_t cap = (uint32_t)cap64;
    if ((rc = S.take(flag, np)) || (rc = S.take(vrank, (size_t)np + 1))) return rc;
    if (check) {  // the verified key table of the model's patterns: the slices of an n-gram are looked up in it, `live` says which still stand
        if ((rc = S.take(table, (size_t)cap64))) return rc;
        Prof prof(c, COLIBRI_K_SKIPGRAM);
        hipLaunchKernelGGL(constraint_clear_kernel, dim3(stream_grid(cap)), dim3(kBlock), 0, c->stream, table.p, cap);
        hipLaunchKernelGGL(constraint_insert_kernel, dim3(stream_grid(np)), dim3(kBlock), 0, c->stream, V.kbytes, V.koff, np, table.p, cap, ~0ull);
    }
    for (uint32_t n = 3; n <= (uint32_t)maxlength; ++n) {
        ms.orders = n - 2;
        if (n > top) break;  // (no pattern is that long: none found)
        const std::vector<uint32_t> masks = gap_masks((int)n, maxskips);
        unsigned long long          nvalid = 0;
        {
            Prof prof(c, COLIBRI_K_SKIPGRAM);
            hipLaunchKernelGGL(mskip_valid_kernel, dim3(stream_grid(np)), dim3(kBlock), 0, c->stream, ntok.p, live.p, np, n, (int)check, V.kbytes, V.koff, table.p, cap, flag.p);
        }
        if ((rc = mskip_scan(c, COLIBRI_K_SKIPGRAM, flag.p, np, vrank.p, &nvalid))) return rc;
        const uint64_t ncand64 = nvalid * (uint64_t)masks.size();
        if (ncand64 >= 0xFFFFFFF0ull)
            return fail(c, COLIBRI_ERR_OVERFLOW, "modelskip: %llu n-grams of %u tokens under %zu gap masks are %llu candidates (32-bit indexing; they are not chunked)", nvalid, n,
                        masks.size(), (unsigned long long)ncand64);
        if (ncand64 == 0) break;  // none found: the order is not pruned
        const uint32_t ncand = (uint32_t)ncand64, nmasks = (uint32_t)masks.size();
        ms.candidates += ncand;
        // candidates: masked lengths, offsets, bytes
        unsigned long long mb = 0;
        if ((rc = S.take(src, (size_t)nvalid)) || (rc = S.take(masks_d, nmasks)) || (rc = S.take(clen, (size_t)ncand + 1)) || (rc = S.take(moff, (size_t)ncand + 1))) return rc;
        HIP_TRY(c, hipMemcpyAsync(masks_d.p, masks.data(), sizeof(uint32_t) * nmasks, hipMemcpyHostToDevice, c->stream));
        {
            Prof prof(c, COLIBRI_K_SKIPGRAM);
            hipLaunchKernelGGL(mskip_sources_kernel, dim3(stream_grid(np)), dim3(kBlock), 0, c->stream, flag.p, vrank.p, np, src.p);
            hipLaunchKernelGGL(mskip_len_kernel, dim3(stream_grid(ncand)), dim3(kBlock), 0, c->stream, src.p, masks_d.p, nmasks, ncand, V.kbytes, V.koff, clen.p);
        }
        if ((rc = mskip_scan(c, COLIBRI_K_SKIPGRAM, clen.p, ncand, moff.p, &mb))) return rc;  // (the sync also covers the copy of `masks`, which goes out of scope with the order)
        const uint64_t gcap64 = (uint64_t)ncand + (ncand >> 1) + 1024;
        if (gcap64 >= 0xFFFFFFF0ull) return fail(c, COLIBRI_ERR_OVERFLOW, "modelskip: %u candidates exceed the group table's 32-bit slots", ncand);
        const uint32_t gcap = (uint32_t)gcap64;
        if ((rc = S.take(mbytes, (size_t)mb + 16)) || (rc = S.take(gtable, (size_t)gcap64)) || (rc = S.take(slot_of, ncand)) || (rc = S.take(isrep, ncand)) ||
            (rc = S.take(rank, (size_t)ncand + 1)))
            return rc;
        HIP_TRY(c, hipMemsetAsync(mbytes.p + mb, 0, 16, c->stream));  // (the byte compares fetch whole words)
        {
            Prof prof(c, COLIBRI_K_SKIPGRAM);
            hipLaunchKernelGGL(mskip_write_kernel, dim3(stream_grid(ncand)), dim3(kBlock), 0, c->stream, src.p, masks_d.p, nmasks, ncand, V.kbytes, V.koff, moff.p, mbytes.p);
        }
        // groups: hash of the masked bytes, verified against the representative; a collision retries under another seed
        bool grouped = false;
        for (int attempt = 0; attempt < 4 && !grouped; ++attempt) {
            const uint64_t seed = 0xBB67AE8584CAA73Bull + 0x9E3779B97F4A7C15ull * (uint64_t)attempt;
            HIP_TRY(c, hipMemsetAsync(info.p, 0, sizeof(MskipInfo), c->stream));
            {
                Prof prof(c, COLIBRI_K_SKIPGRAM);
                hipLaunchKernelGGL(mskip_clear_kernel, dim3(stream_grid(gcap)), dim3(kBlock), 0, c->stream, gtable.p, gcap);
                hipLaunchKernelGGL(mskip_insert_kernel, dim3(stream_grid(ncand)), dim3(kBlock), 0, c->stream, mbytes.p, moff.p, clen.p, src.p, nmasks, ncand, V.roff, seed,
                                   retry_hash_mask("COLIBRI_MSKIP_HASH_BITS", attempt, 3), gtable.p, gcap, slot_of.p);
                hipLaunchKernelGGL(mskip_verify_kernel, dim3(stream_grid(ncand)), dim3(kBlock), 0, c->stream, mbytes.p, moff.p, clen.p, ncand, gtable.p, slot_of.p, isrep.p, info.p);
            }
            MskipInfo got{};
            HIP_TRY(c, hipMemcpyAsync(&got, info.p, sizeof got, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            HIP_TRY(c, hipGetLastError());
            grouped = !got.collision;
            ms.retries += grouped ? 0 : 1;
        }
        if (!grouped) return fail(c, COLIBRI_ERR_OVERFLOW, "modelskip: hash collisions under four seeds");
        unsigned long long ng = 0, nkept = 0, kb = 0, nk = 0;
        if ((rc = mskip_scan(c, COLIBRI_K_SKIPGRAM, isrep.p, ncand, rank.p, &ng))) return rc;
        const uint32_t G = (uint32_t)ng;  // (> 0: there are candidates)
        if ((rc = S.take(gcnt, G)) || (rc = S.take(gtypes, G)) || (rc = S.take(grep, G)) || (rc = S.take(gkeep, G)) || (rc = S.take(kcnt, G)) || (rc = S.take(klen, G)) ||
            (rc = S.take(krank, (size_t)G + 1)) || (rc = S.take(kkoff, (size_t)G + 1)) || (rc = S.take(kroff, (size_t)G + 1)))
            return rc;
        {
            Prof prof(c, COLIBRI_K_SKIPGRAM);
            hipLaunchKernelGGL(mskip_groups_kernel, dim3(stream_grid(ncand)), dim3(kBlock), 0, c->stream, isrep.p, rank.p, clen.p, gtable.p, slot_of.p, ncand, t, mintypes, gcnt.p,
                               gtypes.p, grep.p, gkeep.p, kcnt.p, klen.p, info.p);
            hipLaunchKernelGGL(mskip_prune_kernel, dim3(stream_grid(np)), dim3(kBlock), 0, c->stream, ntok.p, np, n, V.roff, t, live.p, ms.keep.p, info.p);
        }
        if ((rc = mskip_scan(c, COLIBRI_K_SKIPGRAM, gkeep.p, G, krank.p, &nkept)) || (rc = mskip_scan(c, COLIBRI_K_SKIPGRAM, klen.p, G, kkoff.p, &kb)) ||
            (rc = mskip_scan(c, COLIBRI_K_SKIPGRAM, kcnt.p, G, kroff.p, &nk)))
            return rc;
        MskipInfo got{};
        HIP_TRY(c, hipMemcpyAsync(&got, info.p, sizeof got, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        ms.found[n]  = G;
        ms.pruned[n] = (uint64_t)got.pruned_ngrams + got.pruned_groups;
        ms.extra[n]  = got.extra;
        ms.nerased += got.pruned_ngrams;
        if (nk >= 0xFFFFFFF0ull) return fail(c, COLIBRI_ERR_OVERFLOW, "modelskip: %llu references of the skipgrams of %u tokens exceed 32-bit indexing", nk, n);
        // the surviving groups only: keys, counts, types, and their references merged in ascending (sentence, token) order
        ms.ord.emplace_back();
        auto& o    = ms.ord.back();
        o.ngroups  = nkept;
        o.keybytes = kb;
        o.nrefs    = nk;
        if (nkept == 0) continue;
        if ((rc = dev_alloc(c, o.keys, (size_t)kb + 16)) || (rc = dev_alloc(c, o.keyoff, (size_t)nkept)) || (rc = dev_alloc(c, o.refoff, (size_t)nkept)) ||
            (rc = dev_alloc(c, o.cnt, (size_t)nkept)) || (rc = dev_alloc(c, o.types, (size_t)nkept)) || (rc = dev_alloc(c, o.sentence, (size_t)nk + 1)) ||
            (rc = dev_alloc(c, o.token, (size_t)nk + 1)))
            return rc;
        {
            Prof prof(c, COLIBRI_K_SKIPGRAM);
            hipLaunchKernelGGL(mskip_keys_kernel, dim3(stream_grid(G)), dim3(kBlock), 0, c->stream, mbytes.p, moff.p, clen.p, grep.p, gkeep.p, gcnt.p, gtypes.p, krank.p, kkoff.p, kroff.p,
                               G, o.keys.p, o.keyoff.p, o.refoff.p, o.cnt.p, o.types.p);
        }
        if (nk) {
            if ((rc = S.take(contrib, ncand)) || (rc = S.take(soff, (size_t)ncand + 1)) || (rc = S.take(iref, (size_t)nk)) || (rc = S.take(gref, (size_t)nk)) ||
                (rc = S.take(key[0], (size_t)nk)) || (rc = S.take(key[1], (size_t)nk)) || (rc = S.take(val[0], (size_t)nk)) || (rc = S.take(val[1], (size_t)nk)))
                return rc;
            {
                Prof prof(c, COLIBRI_K_INDEX);
                hipLaunchKernelGGL(mskip_contrib_kernel, dim3(stream_grid(ncand)), dim3(kBlock), 0, c->stream, src.p, nmasks, ncand, V.roff, gtable.p, slot_of.p, rank.p, gkeep.p, contrib.p);
            }
            if ((rc = mskip_scan(c, COLIBRI_K_INDEX, contrib.p, ncand, soff.p, nullptr))) return rc;
            {
                Prof prof(c, COLIBRI_K_INDEX);
                hipLaunchKernelGGL(mskip_ref_list_kernel, dim3(stream_grid(nk)), dim3(kBlock), 0, c->stream, soff.p, contrib.p, ncand, (uint64_t)nk, src.p, nmasks, V.roff, gtable.p,
                                   slot_of.p, rank.p, krank.p, V.rs, V.rt, iref.p, gref.p, key[0].p, val[0].p, info.p);
            }
            HIP_TRY(c, hipMemcpyAsync(&got, info.p, sizeof got, hipMemcpyDeviceToHost, c->stream));  // (the largest sentence number: the middle sort's digits)
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            HIP_TRY(c, hipGetLastError());
            Prof prof(c, COLIBRI_K_INDEX);  // (the sorts and what is between them: nothing below waits for the host)
            uint32_t* const keys[2] = {key[0].p, key[1].p};
            uint32_t* const vals[2] = {val[0].p, val[1].p};
            int             cur     = 0;
            if ((rc = radix_sort_pairs(c, keys, vals, nk, 16, cur))) return rc;
            hipLaunchKernelGGL(mskip_gather_kernel, dim3(stream_grid(nk)), dim3(kBlock), 0, c->stream, V.rs, iref.p, vals[cur], (uint64_t)nk, keys[cur]);
            if ((rc = radix_sort_pairs(c, keys, vals, nk, bits_for((uint64_t)got.maxsentence + 1), cur))) return rc;
            hipLaunchKernelGGL(mskip_gather_kernel, dim3(stream_grid(nk)), dim3(kBlock), 0, c->stream, gref.p, (const uint32_t*)nullptr, vals[cur], (uint64_t)nk, keys[cur]);
            if ((rc = radix_sort_pairs(c, keys, vals, nk, bits_for(nkept), cur))) return rc;
            hipLaunchKernelGGL(mskip_refs_out_kernel, dim3(stream_grid(nk)), dim3(kBlock), 0, c->stream, vals[cur], iref.p, (uint64_t)nk, V.rs, V.rt, o.sentence.p, o.token.p);
        }
        HIP_TRY(c, hipStreamSynchronize(c->stream));  // (the order's scratch is taken again, perhaps moved, by the next order)
        HIP_TRY(c, hipGetLastError());
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    collect_events(c);
    ms.scratch = S.peak;
    return COLIBRI_OK;
}

static int mskip_begin(colibri_ctx* c, int mintokens, int mintokens_skipgrams, int minskiptypes, int maxlength, int maxskips, uint64_t* nskipgrams, uint64_t* keybytes, uint64_t* nrefs,
                       uint64_t* nerased, uint32_t& t, bool& check) {
    if (!c || !nskipgrams || !keybytes || !nrefs || !nerased) return COLIBRI_ERR_ARG;
    auto& ms = c->ms;
    ms.valid = false;
    ms.ord.clear();
    ms.np     = 0;
    ms.orders = maxlength >= 3 ? 1 : 0;  // (an empty model, or one without a pattern of three tokens: order 3 is looked at and finds nothing)
    ms.candidates = ms.scratch = ms.nerased = ms.retries = 0;
    std::fill(std::begin(ms.found), std::end(ms.found), 0);
    std::fill(std::begin(ms.pruned), std::end(ms.pruned), 0);
    std::fill(std::begin(ms.extra), std::end(ms.extra), 0);
    *nskipgrams = *keybytes = *nrefs = *nerased = 0;
    if (mintokens < -1 || maxlength < 0 || maxskips < 0)
        return fail(c, COLIBRI_ERR_ARG, "modelskip: MINTOKENS %d, MAXLENGTH %d, MAXSKIPS %d: MINTOKENS may be -1 (2), the others not negative", mintokens, maxlength, maxskips);
    t     = (uint32_t)(mintokens == -1 ? 2 : mintokens);  // IndexedPatternModel::trainskipgrams, reference include/patternmodel.h:2971-2972
    check = std::max<int64_t>(mintokens_skipgrams, t) > 1;  // computeskipgrams: the slices are only asked for above a threshold of 1
    (void)minskiptypes;
    HIP_TRY(c, hipSetDevice(c->device));
    return COLIBRI_OK;
}
static int mskip_end(colibri_ctx* c, int rc, uint64_t* nskipgrams, uint64_t* keybytes, uint64_t* nrefs, uint64_t* nerased) {
    auto& ms = c->ms;
    if (rc) {
        ms.ord.clear();
        return rc;
    }
    for (const auto& o : ms.ord) {
        *nskipgrams += o.ngroups;
        *keybytes += o.keybytes;
        *nrefs += o.nrefs;
    }
    *nerased = ms.nerased;
    ms.valid = true;
    return COLIBRI_OK;
}

int colibri_modelskip(colibri_ctx* c, const uint64_t* key_off, const uint8_t* key_bytes, const uint64_t* ref_off, const uint32_t* ref_sentence, const uint16_t* ref_token,
                      uint64_t npatterns, int mintokens, int mintokens_skipgrams, int minskiptypes, int maxlength, int maxskips, uint64_t* nskipgrams, uint64_t* keybytes,
                      uint64_t* nrefs, uint64_t* nerased) {
    uint32_t t     = 0;
    bool     check = false;
    int      rc    = mskip_begin(c, mintokens, mintokens_skipgrams, minskiptypes, maxlength, maxskips, nskipgrams, keybytes, nrefs, nerased, t, check);
    if (rc) return rc;
    if (npatterns == 0) {
        c->ms.valid = true;
        return COLIBRI_OK;
    }
    ModelView V;
    if ((rc = model_upload(c, "modelskip", key_off, key_bytes, nullptr, ref_off, ref_sentence, ref_token, npatterns, kModelIndexed, V))) return rc;
    if ((rc = dev_alloc(c, c->ms.keep, V.np))) return rc;
    c->ms.np = V.np;
    return mskip_end(c, mskip_core(c, V, t, check, (uint32_t)std::max(minskiptypes, 0), maxlength, maxskips), nskipgrams, keybytes, nrefs, nerased);
}

// the same on the indexed model of the last colibri_train of this context, where it lies in HBM; nothing of the context's model is written
int colibri_modelskip_resident(colibri_ctx* c, int mintokens, int mintokens_skipgrams, int minskiptypes, int maxlength, int maxskips, uint64_t* nskipgrams, uint64_t* keybytes,
                               uint64_t* nrefs, uint64_t* nerased) {
    uint32_t t     = 0;
    bool     check = false;
    int      rc    = mskip_begin(c, mintokens, mintokens_skipgrams, minskiptypes, maxlength, maxskips, nskipgrams, keybytes, nrefs, nerased, t, check);
    if (rc) return rc;
    ModelView V;
    if ((rc = model_resident(c, "colibri_modelskip_resident", true, V))) return rc;
    if (V.np == 0) {
        c->ms.valid = true;
        return COLIBRI_OK;
    }
    if ((rc = dev_alloc(c, c->ms.keep, V.np))) return rc;
    c->ms.np = V.np;
    return mskip_end(c, mskip_core(c, V, t, check, (uint32_t)std::max(minskiptypes, 0), maxlength, maxskips), nskipgrams, keybytes, nrefs, nerased);
}

// key_off / ref_off: nskipgrams + 1 entries; counts / types: nskipgrams; keep: one byte per pattern of the model (1 = it stays), in the order of its arrays
int colibri_modelskip_fetch(colibri_ctx* c, uint64_t* key_off, uint8_t* key_bytes, uint32_t* counts, uint32_t* types, uint64_t* ref_off, uint32_t* ref_sentence, uint16_t* ref_token,
                            uint8_t* keep) {
    if (!c || !key_off || !ref_off) return COLIBRI_ERR_ARG;
    auto& ms = c->ms;
    if (!ms.valid) return fail(c, COLIBRI_ERR_STATE, "colibri_modelskip / colibri_modelskip_resident first");
    HIP_TRY(c, hipSetDevice(c->device));
    uint64_t g0 = 0, k0 = 0, r0 = 0;
    for (const auto& o : ms.ord) {
        const uint64_t G = o.ngroups;
        if (G) {
            if (!key_bytes || !counts || !types || (o.nrefs && (!ref_sentence || !ref_token))) return COLIBRI_ERR_ARG;
            HIP_TRY(c, hipMemcpyAsync(key_off + g0, o.keyoff.p, sizeof(uint64_t) * G, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipMemcpyAsync(ref_off + g0, o.refoff.p, sizeof(uint64_t) * G, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipMemcpyAsync(counts + g0, o.cnt.p, sizeof(uint32_t) * G, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipMemcpyAsync(types + g0, o.types.p, sizeof(uint32_t) * G, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipMemcpyAsync(key_bytes + k0, o.keys.p, o.keybytes, hipMemcpyDeviceToHost, c->stream));
            if (o.nrefs) {
                HIP_TRY(c, hipMemcpyAsync(ref_sentence + r0, o.sentence.p, sizeof(uint32_t) * o.nrefs, hipMemcpyDeviceToHost, c->stream));
                HIP_TRY(c, hipMemcpyAsync(ref_token + r0, o.token.p, sizeof(uint16_t) * o.nrefs, hipMemcpyDeviceToHost, c->stream));
            }
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            for (uint64_t g = g0; g < g0 + G; ++g) {  // an order's offsets are its own: behind the orders before it
                key_off[g] += k0;
                ref_off[g] += r0;
            }
        }
        g0 += G, k0 += o.keybytes, r0 += o.nrefs;
    }
    key_off[g0] = k0;
    ref_off[g0] = r0;
    if (keep && ms.np) {
        HIP_TRY(c, hipMemcpyAsync(keep, ms.keep.p, ms.np, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    return COLIBRI_OK;
}

// what the last call did. *orders: the orders it looked at, 3 .. *orders + 2 (the last may have found nothing: the loop ended there);
// found / pruned / extra: COLIBRI_MAX_ORDER entries by the order n; any may be NULL
int colibri_modelskip_info(const colibri_ctx* c, uint32_t* orders, uint64_t* found, uint64_t* pruned, uint64_t* extra, uint64_t* candidates, uint64_t* scratch_bytes) {
    if (!c) return COLIBRI_ERR_ARG;
    const auto& ms = c->ms;
    if (orders) *orders = ms.orders;
    if (found) std::copy(std::begin(ms.found), std::end(ms.found), found);
    if (pruned) std::copy(std::begin(ms.pruned), std::end(ms.pruned), pruned);
    if (extra) std::copy(std::begin(ms.extra), std::end(ms.extra), extra);
    if (candidates) *candidates = ms.candidates;
    if (scratch_bytes) *scratch_bytes = ms.scratch;
    return COLIBRI_OK;
}
