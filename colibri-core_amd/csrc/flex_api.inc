// flex_api.inc — part of colibri_hip.hip (included there, inside its extern "C" block): flexgrams abstracted from the skipgrams
// of an indexed model (SURVEY §8 f-4; kernels and the specification in flexgrams.hpp).
// the device pipeline on a model already in HBM: kbytes / koff (np + 1) / roff (np + 1) / rs / rt (nr_in references)
static int flex_core(colibri_ctx* c, const uint8_t* kbytes_p, const unsigned long long* koff_p, const unsigned long long* roff_p, const uint32_t* rs_p, const uint16_t* rt_p, uint32_t np,
                     uint64_t nr_in, uint64_t* nflexgrams, uint64_t* keybytes, uint64_t* nrefs) {
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
        hipLaunchKernelGGL(flex_len_kernel, dim3(stream_grid(np)), dim3(kBlock), 0, c->stream, kbytes_p, koff_p, np, flen.p);
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
    hipLaunchKernelGGL(flex_write_kernel, dim3(stream_grid(np)), dim3(kBlock), 0, c->stream, kbytes_p, koff_p, np, flen.p, foff.p, fbytes.p);
    // groups: hash of the collapsed bytes, verified against the representative; a collision retries under another seed
    bool grouped = false;
    for (int attempt = 0; attempt < 4 && !grouped; ++attempt) {
        const uint64_t seed = 0x6A09E667F3BCC909ull + 0x9E3779B97F4A7C15ull * (uint64_t)attempt;
        HIP_TRY(c, hipMemsetAsync(info.p, 0, sizeof(FlexInfo), c->stream));
        {
            Prof p(c, COLIBRI_K_SKIPGRAM);
            hipLaunchKernelGGL(flex_clear_kernel, dim3(stream_grid(cap)), dim3(kBlock), 0, c->stream, table.p, cap);
            hipLaunchKernelGGL(flex_insert_kernel, dim3(stream_grid(np)), dim3(kBlock), 0, c->stream, fbytes.p, foff.p, flen.p, roff_p, np, seed, table.p, cap, slot_of.p,
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
        hipLaunchKernelGGL(flex_contrib_kernel, dim3(stream_grid(np)), dim3(kBlock), 0, c->stream, flen.p, roff_p, np, contrib.p);
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
        hipLaunchKernelGGL(flex_ref_list_kernel, dim3(stream_grid(nr_in)), dim3(kBlock), 0, c->stream, roff_p, np, nr_in, flen.p, soff.p, table.p, slot_of.p, rank.p, rs_p, rt_p, gref.p,
                           key[0].p, val[0].p, info.p);
        FlexInfo got{};
        HIP_TRY(c, hipMemcpyAsync(&got, info.p, sizeof got, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        HIP_TRY(c, hipGetLastError());
        uint32_t* const keys[2] = {key[0].p, key[1].p};
        uint32_t* const vals[2] = {val[0].p, val[1].p};
        int             cur     = 0;
        if ((rc = radix_sort_pairs(c, keys, vals, nf, 16, cur))) return rc;
        hipLaunchKernelGGL(flex_gather_kernel, dim3(stream_grid(nf)), dim3(kBlock), 0, c->stream, rs_p, vals[cur], nf, keys[cur]);
        if ((rc = radix_sort_pairs(c, keys, vals, nf, bits_for((uint64_t)got.maxsentence + 1), cur))) return rc;
        hipLaunchKernelGGL(flex_gather_kernel, dim3(stream_grid(nf)), dim3(kBlock), 0, c->stream, gref.p, vals[cur], nf, keys[cur]);
        if ((rc = radix_sort_pairs(c, keys, vals, nf, bits_for(G), cur))) return rc;
        hipLaunchKernelGGL(flex_refs_out_kernel, dim3(stream_grid(nf)), dim3(kBlock), 0, c->stream, vals[cur], nf, rs_p, rt_p, fx.sentence.p, fx.token.p);
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

int colibri_flexgrams(colibri_ctx* c, const uint64_t* key_off, const uint8_t* key_bytes, const uint64_t* ref_off, const uint32_t* ref_sentence, const uint16_t* ref_token,
                      uint64_t npatterns, uint64_t* nflexgrams, uint64_t* keybytes, uint64_t* nrefs) {
    if (!c || !nflexgrams || !keybytes || !nrefs) return COLIBRI_ERR_ARG;
    auto& fx      = c->fx;
    fx.valid      = false;
    fx.ngroups    = fx.keybytes = fx.nrefs = 0;
    *nflexgrams   = *keybytes = *nrefs = 0;
    if (npatterns == 0) {
        fx.valid = true;
        return COLIBRI_OK;
    }
    if (!key_off || !key_bytes || !ref_off) return COLIBRI_ERR_ARG;
    const uint64_t nb_in = key_off[npatterns], nr_in = ref_off[npatterns];
    if (nr_in && (!ref_sentence || !ref_token)) return COLIBRI_ERR_ARG;
    if (npatterns >= 0x7FFFFFF0ull || nr_in >= 0xFFFFFFF0ull) return fail(c, COLIBRI_ERR_OVERFLOW, "flexgrams: %llu patterns / %llu references exceed 32-bit indexing",
                                                                          (unsigned long long)npatterns, (unsigned long long)nr_in);
    HIP_TRY(c, hipSetDevice(c->device));
    const uint32_t np = (uint32_t)npatterns;
    int            rc;
    // the model on the device
    DevBuf<uint8_t>            kbytes;
    DevBuf<unsigned long long> koff, roff;
    DevBuf<uint32_t>           rs;
    DevBuf<uint16_t>           rt;
    if ((rc = dev_alloc(c, kbytes, (size_t)nb_in + 16)) || (rc = dev_alloc(c, koff, (size_t)np + 1)) || (rc = dev_alloc(c, roff, (size_t)np + 1)) ||
        (rc = dev_alloc(c, rs, (size_t)nr_in + 1)) || (rc = dev_alloc(c, rt, (size_t)nr_in + 1)))
        return rc;
    if (nb_in) HIP_TRY(c, hipMemcpyAsync(kbytes.p, key_bytes, nb_in, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(koff.p, key_off, sizeof(uint64_t) * ((size_t)np + 1), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(roff.p, ref_off, sizeof(uint64_t) * ((size_t)np + 1), hipMemcpyHostToDevice, c->stream));
    if (nr_in) {
        HIP_TRY(c, hipMemcpyAsync(rs.p, ref_sentence, sizeof(uint32_t) * nr_in, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(rt.p, ref_token, sizeof(uint16_t) * nr_in, hipMemcpyHostToDevice, c->stream));
    }
    return flex_core(c, kbytes.p, koff.p, roff.p, rs.p, rt.p, np, nr_in, nflexgrams, keybytes, nrefs);
}

// the same on the indexed model of the last colibri_train of this context, which is still resident in HBM: no host round trip
int colibri_flexgrams_resident(colibri_ctx* c, uint64_t* nflexgrams, uint64_t* keybytes, uint64_t* nrefs) {
    if (!c || !nflexgrams || !keybytes || !nrefs) return COLIBRI_ERR_ARG;
    auto& fx      = c->fx;
    fx.valid      = false;
    fx.ngroups    = fx.keybytes = fx.nrefs = 0;
    *nflexgrams   = *keybytes = *nrefs = 0;
    if (!c->trained || !c->opt.indexed || c->sh.active) return fail(c, COLIBRI_ERR_STATE, "colibri_flexgrams_resident needs the indexed model of a colibri_train on this context");
    const uint32_t R = c->hstate.res_total;
    if (R == 0) {
        fx.valid = true;
        return COLIBRI_OK;
    }
    if (c->npairs >= 0xFFFFFFF0ull) return fail(c, COLIBRI_ERR_OVERFLOW, "flexgrams: %llu references exceed 32-bit indexing", (unsigned long long)c->npairs);
    HIP_TRY(c, hipSetDevice(c->device));
    int                        rc;
    if ((rc = ensure_export(c))) return rc;  // key lengths / offsets of the resident model
    DevBuf<uint8_t>            kbytes;
    DevBuf<unsigned long long> roff;
    if ((rc = dev_alloc(c, kbytes, (size_t)c->keybytes + 16)) || (rc = dev_alloc(c, roff, (size_t)R + 1))) return rc;
    {
        Prof p(c, COLIBRI_K_EXPORT);
        for (const auto& sg : c->segments)
            hipLaunchKernelGGL(export_bytes_kernel, dim3(blocks_for(sg.count, kBlock)), dim3(kBlock), 0, c->stream, c->bytes.p, c->tokstart.p, c->res_rep.p, c->keylen.p, c->keyoff.p,
                               sg.first, sg.count, sg.n, sg.mask, kbytes.p);
    }
    const unsigned long long kb_total = c->keybytes, nr_total = c->npairs;
    HIP_TRY(c, hipMemcpyAsync(c->keyoff.p + R, &kb_total, sizeof kb_total, hipMemcpyHostToDevice, c->stream));  // keyoff holds R offsets: close the range
    if ((rc = scan_u32(c, c->res_cnt.p, R, roff.p, nullptr))) return rc;
    HIP_TRY(c, hipMemcpyAsync(roff.p + R, &nr_total, sizeof nr_total, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // the two host words above are read by the copies
    return flex_core(c, kbytes.p, c->keyoff.p, roff.p, c->ref_sentence.p, c->ref_token.p, R, c->npairs, nflexgrams, keybytes, nrefs);
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
