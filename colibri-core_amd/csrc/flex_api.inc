// flex_api.inc — part of colibri_hip.hip (included there, inside its extern "C" block): flexgrams abstracted from the skipgrams
// of an indexed model (SURVEY §8 f-4; kernels and the specification in flexgrams.hpp).
// the device pipeline on an indexed model in HBM
static int flex_core(colibri_ctx* c, const ModelView& V, uint64_t* nflexgrams, uint64_t* keybytes, uint64_t* nrefs) {
    const uint32_t np    = V.np;
    const uint64_t nr_in = V.nrefs;
    auto& fx = c->fx;
    int   rc;
    DevBuf<uint8_t>            fbytes;
    DevBuf<unsigned long long> foff, rank, soff;
    DevBuf<uint32_t>           flen, slot_of, isrep, contrib, grep, glen, gref, key[2], val[2];
    DevBuf<FSlot>              table;
    DevBuf<FlexInfo>           info;
    if ((rc = dev_alloc(c, flen, (size_t)np + 1)) || (rc = dev_alloc(c, foff, (size_t)np + 1)) || (rc = dev_alloc(c, info, 1))) return rc;
    // collapsed keys
    unsigned long long fb = 0;
    {
        Prof p(c, COLIBRI_K_SKIPGRAM);
        hipLaunchKernelGGL(flex_len_kernel, dim3(stream_grid(np)), dim3(kBlock), 0, c->stream, V.kbytes, V.koff, np, flen.p);
    }
    if ((rc = scan_u32(c, flen.p, np, foff.p, &fb))) return rc;
    if (fb == 0) {  // no skipgrams: no flexgrams
        fx.valid = true;
        return COLIBRI_OK;
    }
    const uint64_t cap64 = (uint64_t)np + (np >> 1) + 1024;
    if ((rc = dev_alloc(c, fbytes, (size_t)fb + 16)) || (rc = dev_alloc(c, table, (size_t)cap64)) || (rc = dev_alloc(c, slot_of, (size_t)np + 1)) ||
        (rc = dev_alloc(c, isrep, (size_t)np + 1)) || (rc = dev_alloc(c, rank, (size_t)np + 1)))
        return rc;
    const uint32_t cap = (uint32_t)cap64;
    hipLaunchKernelGGL(flex_write_kernel, dim3(stream_grid(np)), dim3(kBlock), 0, c->stream, V.kbytes, V.koff, np, flen.p, foff.p, fbytes.p);
    // groups: hash of the collapsed bytes, verified against the representative; a collision retries under another seed
    bool grouped = false;
    for (int attempt = 0; attempt < 4 && !grouped; ++attempt) {
        const uint64_t seed = 0x6A09E667F3BCC909ull + 0x9E3779B97F4A7C15ull * (uint64_t)attempt;
        HIP_TRY(c, hipMemsetAsync(info.p, 0, sizeof(FlexInfo), c->stream));
        {
            Prof p(c, COLIBRI_K_SKIPGRAM);
            hipLaunchKernelGGL(flex_clear_kernel, dim3(stream_grid(cap)), dim3(kBlock), 0, c->stream, table.p, cap);
            hipLaunchKernelGGL(flex_insert_kernel, dim3(stream_grid(np)), dim3(kBlock), 0, c->stream, fbytes.p, foff.p, flen.p, V.roff, np, seed, table.p, cap, slot_of.p,
                               retry_hash_mask("COLIBRI_FLEX_HASH_BITS", attempt));
            hipLaunchKernelGGL(flex_verify_kernel, dim3(stream_grid(np)), dim3(kBlock), 0, c->stream, fbytes.p, foff.p, flen.p, np, table.p, slot_of.p, isrep.p, info.p);
        }
        FlexInfo got{};
        HIP_TRY(c, hipMemcpyAsync(&got, info.p, sizeof got, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        HIP_TRY(c, hipGetLastError());
        grouped = !got.collision;
    }
    if (!grouped) return fail(c, COLIBRI_ERR_OVERFLOW, "flexgrams: hash collisions under four seeds");
    unsigned long long ng = 0, nf = 0, kb = 0;
    if ((rc = scan_u32(c, isrep.p, np, rank.p, &ng))) return rc;
    const uint32_t G = (uint32_t)ng;
    if ((rc = dev_alloc(c, fx.cnt, (size_t)G + 1)) || (rc = dev_alloc(c, glen, (size_t)G + 1)) || (rc = dev_alloc(c, grep, (size_t)G + 1)) ||
        (rc = dev_alloc(c, fx.keyoff, (size_t)G + 1)) || (rc = dev_alloc(c, fx.refoff, (size_t)G + 1)) || (rc = dev_alloc(c, contrib, (size_t)np + 1)) ||
        (rc = dev_alloc(c, soff, (size_t)np + 1)))
        return rc;
    {
        Prof p(c, COLIBRI_K_SKIPGRAM);
        hipLaunchKernelGGL(flex_groups_kernel, dim3(stream_grid(np)), dim3(kBlock), 0, c->stream, isrep.p, rank.p, flen.p, table.p, slot_of.p, np, fx.cnt.p, glen.p, grep.p);
        hipLaunchKernelGGL(flex_contrib_kernel, dim3(stream_grid(np)), dim3(kBlock), 0, c->stream, flen.p, V.roff, np, contrib.p);
    }
    if ((rc = scan_u32(c, fx.cnt.p, G, fx.refoff.p, &nf)) || (rc = scan_u32(c, glen.p, G, fx.keyoff.p, &kb)) || (rc = scan_u32(c, contrib.p, np, soff.p, nullptr))) return rc;
    if ((rc = dev_alloc(c, fx.keys, (size_t)kb + 16)) || (rc = dev_alloc(c, fx.sentence, (size_t)nf + 1)) || (rc = dev_alloc(c, fx.token, (size_t)nf + 1))) return rc;
    hipLaunchKernelGGL(flex_keys_kernel, dim3(stream_grid(G)), dim3(kBlock), 0, c->stream, fbytes.p, foff.p, grep.p, glen.p, fx.keyoff.p, G, fx.keys.p);
    // merged reference lists: sort the skipgram references by (group, sentence, token)
    if (nf) {
        if ((rc = dev_alloc(c, gref, (size_t)nr_in + 1)) || (rc = dev_alloc(c, key[0], (size_t)nf)) || (rc = dev_alloc(c, key[1], (size_t)nf)) ||
            (rc = dev_alloc(c, val[0], (size_t)nf)) || (rc = dev_alloc(c, val[1], (size_t)nf)))
            return rc;
        Prof p(c, COLIBRI_K_INDEX);
        hipLaunchKernelGGL(flex_ref_list_kernel, dim3(stream_grid(nr_in)), dim3(kBlock), 0, c->stream, V.roff, np, nr_in, flen.p, soff.p, table.p, slot_of.p, rank.p, V.rs, V.rt, gref.p,
                           key[0].p, val[0].p, info.p);
        FlexInfo got{};
        HIP_TRY(c, hipMemcpyAsync(&got, info.p, sizeof got, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        HIP_TRY(c, hipGetLastError());
        uint32_t* const keys[2] = {key[0].p, key[1].p};
        uint32_t* const vals[2] = {val[0].p, val[1].p};
        int             cur     = 0;
        if ((rc = radix_sort_pairs(c, keys, vals, nf, 16, cur))) return rc;
        hipLaunchKernelGGL(flex_gather_kernel, dim3(stream_grid(nf)), dim3(kBlock), 0, c->stream, V.rs, vals[cur], nf, keys[cur]);
        if ((rc = radix_sort_pairs(c, keys, vals, nf, bits_for((uint64_t)got.maxsentence + 1), cur))) return rc;
        hipLaunchKernelGGL(flex_gather_kernel, dim3(stream_grid(nf)), dim3(kBlock), 0, c->stream, gref.p, vals[cur], nf, keys[cur]);
        if ((rc = radix_sort_pairs(c, keys, vals, nf, bits_for(G), cur))) return rc;
        hipLaunchKernelGGL(flex_refs_out_kernel, dim3(stream_grid(nf)), dim3(kBlock), 0, c->stream, vals[cur], nf, V.rs, V.rt, fx.sentence.p, fx.token.p);
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    collect_events(c);
    fx.ngroups  = G;
    fx.keybytes = kb;
    fx.nrefs    = nf;
    fx.valid    = true;
    *nflexgrams = G;
    *keybytes   = kb;
    *nrefs      = nf;
    return COLIBRI_OK;
}

static int flex_begin(colibri_ctx* c, uint64_t* nflexgrams, uint64_t* keybytes, uint64_t* nrefs) {
    if (!c || !nflexgrams || !keybytes || !nrefs) return COLIBRI_ERR_ARG;
    auto& fx      = c->fx;
    fx.valid      = false;
    fx.ngroups    = fx.keybytes = fx.nrefs = 0;
    *nflexgrams   = *keybytes = *nrefs = 0;
    return COLIBRI_OK;
}

int colibri_flexgrams(colibri_ctx* c, const uint64_t* key_off, const uint8_t* key_bytes, const uint64_t* ref_off, const uint32_t* ref_sentence, const uint16_t* ref_token,
                      uint64_t npatterns, uint64_t* nflexgrams, uint64_t* keybytes, uint64_t* nrefs) {
    int rc = flex_begin(c, nflexgrams, keybytes, nrefs);
    if (rc) return rc;
    if (npatterns == 0) {
        c->fx.valid = true;
        return COLIBRI_OK;
    }
    ModelView V;
    if ((rc = model_upload(c, "flexgrams", key_off, key_bytes, nullptr, ref_off, ref_sentence, ref_token, npatterns, kModelIndexed, V))) return rc;
    return flex_core(c, V, nflexgrams, keybytes, nrefs);
}

// the same on the indexed model of the last colibri_train of this context, which is still resident in HBM: no host round trip
int colibri_flexgrams_resident(colibri_ctx* c, uint64_t* nflexgrams, uint64_t* keybytes, uint64_t* nrefs) {
    int rc = flex_begin(c, nflexgrams, keybytes, nrefs);
    if (rc) return rc;
    ModelView V;
    if ((rc = model_resident(c, "colibri_flexgrams_resident", true, V))) return rc;
    if (V.np == 0) {
        c->fx.valid = true;
        return COLIBRI_OK;
    }
    return flex_core(c, V, nflexgrams, keybytes, nrefs);
}

int colibri_flexgrams_fetch(colibri_ctx* c, uint64_t* key_off, uint8_t* key_bytes, uint32_t* counts, uint64_t* ref_off, uint32_t* ref_sentence, uint16_t* ref_token) {
    if (!c || !key_off || !ref_off) return COLIBRI_ERR_ARG;
    auto& fx = c->fx;
    if (!fx.valid) return fail(c, COLIBRI_ERR_STATE, "colibri_flexgrams first");
    const uint64_t G = fx.ngroups;
    key_off[G]       = fx.keybytes;
    ref_off[G]       = fx.nrefs;
    if (!G) return COLIBRI_OK;
    if (!key_bytes || !counts || (fx.nrefs && (!ref_sentence || !ref_token))) return COLIBRI_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(key_off, fx.keyoff.p, sizeof(uint64_t) * G, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(ref_off, fx.refoff.p, sizeof(uint64_t) * G, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(counts, fx.cnt.p, sizeof(uint32_t) * G, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(key_bytes, fx.keys.p, fx.keybytes, hipMemcpyDeviceToHost, c->stream));
    if (fx.nrefs) {
        HIP_TRY(c, hipMemcpyAsync(ref_sentence, fx.sentence.p, sizeof(uint32_t) * fx.nrefs, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(ref_token, fx.token.p, sizeof(uint16_t) * fx.nrefs, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return COLIBRI_OK;
}
