// compare_api.inc — part of colibri_hip.hip (included there, inside its extern "C" block, after cooc_api.inc): log-likelihood comparison of
// N >= 2 pattern models (colibri-comparemodels; kernels and the specification in compare.hpp).

int colibri_compare(colibri_ctx* c, int nmodels, const uint64_t* const* key_off, const uint8_t* const* key_bytes, const uint32_t* const* counts, const uint64_t* npatterns,
                    const uint64_t* tokens, int flags, uint64_t* nrows) {
    if (!c || !nrows || nmodels < 2 || !key_off || !key_bytes || !counts || !npatterns || !tokens) return COLIBRI_ERR_ARG;
    if (flags & ~(COLIBRI_COMPARE_CONJUNCTION | COLIBRI_COMPARE_UNSORTED)) return COLIBRI_ERR_ARG;
    auto& cm = c->cm;
    cm.valid = false;
    cm.nrows = cm.distinct = cm.scratch = 0;
    cm.nmodels = (uint32_t)nmodels;
    *nrows     = 0;
    const uint32_t nm = (uint32_t)nmodels;
    uint64_t       T64 = 0, B64 = 0;
    std::vector<uint32_t> hstart(nm + 1);
    std::vector<int>      htok(nm);
    for (uint32_t m = 0; m < nm; ++m) {
        if (npatterns[m] && (!key_off[m] || !key_bytes[m] || !counts[m])) return COLIBRI_ERR_ARG;
        if (tokens[m] > 0x7FFFFFFFull)
            return fail(c, COLIBRI_ERR_OVERFLOW, "compare: model %u has %llu tokens, more than INT_MAX (the reference's int totals would wrap)", m, (unsigned long long)tokens[m]);
        htok[m]   = (int)tokens[m];
        hstart[m] = (uint32_t)T64;
        T64 += npatterns[m];
        B64 += npatterns[m] ? key_off[m][npatterns[m]] : 0;
        if (T64 >= 0x7FFFFFF0ull) return fail(c, COLIBRI_ERR_OVERFLOW, "compare: %llu patterns in all exceed 32-bit indexing", (unsigned long long)T64);
    }
    hstart[nm] = (uint32_t)T64;
    if (T64 == 0) {
        cm.valid = true;
        return COLIBRI_OK;
    }
    const uint32_t T    = (uint32_t)T64;
    const int      conj = (flags & COLIBRI_COMPARE_CONJUNCTION) != 0, sorted = (flags & COLIBRI_COMPARE_UNSORTED) == 0;
    const uint64_t hmask = env_hash_mask("COLIBRI_COMPARE_HASH_BITS");  // (tests: a hash of a few bits, so that byte checks decide identity)
    HIP_TRY(c, hipSetDevice(c->device));
    int         rc;
    DevScratch  S{c};
    DevBuf<uint8_t>            kbytes, cat;
    DevBuf<unsigned long long> koff, did, kofs, tot;
    DevBuf<uint32_t>           cnt, mstart, info, rep, head, observed, rowg, keep, kd, kg, perm[2], key[2];
    DevBuf<uint64_t>           hash;
    DevBuf<uint16_t>           ntok;
    DevBuf<int>                tok;
    DevBuf<CSlot>              table;
    DevBuf<double>             ll;
    // the models' keys, concatenated: bytes, offsets shifted to the whole, counts
    if ((rc = S.take(kbytes, (size_t)B64 + 16)) || (rc = S.take(koff, (size_t)T + 1)) || (rc = S.take(cnt, (size_t)T)) || (rc = S.take(mstart, (size_t)nm + 1)) ||
        (rc = S.take(tok, nm)) || (rc = S.take(info, 2)))
        return rc;
    HIP_TRY(c, hipMemsetAsync(kbytes.p + B64, 0, 16, c->stream));
    HIP_TRY(c, hipMemsetAsync(info.p, 0, 2 * sizeof(uint32_t), c->stream));
    HIP_TRY(c, hipMemcpyAsync(mstart.p, hstart.data(), sizeof(uint32_t) * (nm + 1), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(tok.p, htok.data(), sizeof(int) * nm, hipMemcpyHostToDevice, c->stream));
    {
        uint64_t b = 0;
        for (uint32_t m = 0; m < nm; ++m) {
            const uint64_t np = npatterns[m];
            if (!np) continue;
            const uint64_t nb = key_off[m][np];
            if (nb) HIP_TRY(c, hipMemcpyAsync(kbytes.p + b, key_bytes[m], nb, hipMemcpyHostToDevice, c->stream));
            HIP_TRY(c, hipMemcpyAsync(koff.p + hstart[m], key_off[m], sizeof(uint64_t) * np, hipMemcpyHostToDevice, c->stream));
            HIP_TRY(c, hipMemcpyAsync(cnt.p + hstart[m], counts[m], sizeof(uint32_t) * np, hipMemcpyHostToDevice, c->stream));
            if (b) hipLaunchKernelGGL(cmp_shift_kernel, dim3(stream_grid(np)), dim3(kBlock), 0, c->stream, koff.p + hstart[m], (uint32_t)np, (unsigned long long)b);
            b += nb;
        }
        const unsigned long long end = b;
        HIP_TRY(c, hipMemcpyAsync(koff.p + T, &end, sizeof end, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));  // (`end` is a host local)
    }
    // (a) identity: hashes into one table, every key's representative by byte checks along its probe chain, the distinct patterns numbered
    const uint64_t cap64 = 2ull * T + 1024;
    if ((rc = S.take(hash, T)) || (rc = S.take(ntok, T)) || (rc = S.take(cat, T)) || (rc = S.take(table, (size_t)cap64)) || (rc = S.take(rep, T))) return rc;
    const uint32_t cap = (uint32_t)cap64;
    uint32_t       hinfo[2];
    {
        Prof p(c, COLIBRI_K_COUNT);
        hipLaunchKernelGGL(cmp_info_kernel, dim3(stream_grid(T)), dim3(kBlock), 0, c->stream, kbytes.p, koff.p, T, hmask, hash.p, ntok.p, cat.p, info.p);
        hipLaunchKernelGGL(constraint_clear_kernel, dim3(stream_grid(cap)), dim3(kBlock), 0, c->stream, table.p, cap);
        hipLaunchKernelGGL(cmp_insert_kernel, dim3(stream_grid(T)), dim3(kBlock), 0, c->stream, hash.p, koff.p, T, table.p, cap);
        hipLaunchKernelGGL(cmp_rep_kernel, dim3(stream_grid(T)), dim3(kBlock), 0, c->stream, kbytes.p, koff.p, hash.p, T, table.p, cap, rep.p);
    }
    HIP_TRY(c, hipMemcpyAsync(hinfo, info.p, sizeof hinfo, hipMemcpyDeviceToHost, c->stream));
    S.drop(table);
    S.drop(hash);
    unsigned long long D = 0;
    if ((rc = S.take(head, (size_t)T + 1)) || (rc = S.take(did, (size_t)T + 1))) return rc;
    hipLaunchKernelGGL(cmp_head_kernel, dim3(stream_grid(T)), dim3(kBlock), 0, c->stream, rep.p, T, head.p);
    HIP_TRY(c, hipMemsetAsync(head.p + T, 0, sizeof(uint32_t), c->stream));
    if ((rc = scan_u32(c, head.p, T + 1, did.p, &D))) return rc;  // (synchronises: hinfo is in)
    S.drop(head);
    const uint32_t maxkey = hinfo[0], G = hinfo[1] + 1;
    // (b) observed counts per (distinct pattern, model), the per-(model, category, size) occurrence totals
    const uint64_t ntot = 4ull * nm * G;
    if ((rc = S.take(observed, (size_t)D * nm)) || (rc = S.take(rowg, (size_t)D)) || (rc = S.take(tot, (size_t)ntot))) return rc;
    HIP_TRY(c, hipMemsetAsync(observed.p, 0, sizeof(uint32_t) * D * nm, c->stream));
    HIP_TRY(c, hipMemsetAsync(tot.p, 0, sizeof(unsigned long long) * ntot, c->stream));
    {
        const bool lds = ntot * sizeof(unsigned long long) <= 32768;
        hipLaunchKernelGGL(cmp_scatter_kernel, dim3(stream_grid(T)), dim3(kBlock), lds ? (size_t)ntot * sizeof(unsigned long long) : 0, c->stream, rep.p, did.p, cnt.p, ntok.p, cat.p,
                           mstart.p, nm, T, G, (int)lds, observed.p, rowg.p, tot.p);
    }
    S.drop(rep);
    S.drop(did);
    S.drop(cnt);
    // (c) ll per distinct pattern, the -a filter, the kept rows compacted
    unsigned long long K = 0;
    if ((rc = S.take(ll, (size_t)D)) || (rc = S.take(keep, (size_t)D + 1)) || (rc = S.take(kofs, (size_t)D + 1))) return rc;
    hipLaunchKernelGGL(cmp_ll_kernel, dim3(stream_grid(D)), dim3(kBlock), 0, c->stream, observed.p, tok.p, nm, (uint32_t)D, conj, ll.p, keep.p);
    HIP_TRY(c, hipMemsetAsync(keep.p + D, 0, sizeof(uint32_t), c->stream));
    if ((rc = scan_u32(c, keep.p, (uint32_t)D + 1, kofs.p, &K))) return rc;
    if ((rc = S.take(kd, (size_t)K + 1)) || (rc = S.take(kg, (size_t)K + 1))) return rc;
    hipLaunchKernelGGL(cmp_compact_kernel, dim3(stream_grid(D)), dim3(kBlock), 0, c->stream, keep.p, kofs.p, rowg.p, (uint32_t)D, kd.p, kg.p);
    S.drop(keep);
    S.drop(kofs);
    S.drop(rowg);
    // (d) the order: key bytes (LSD: length, then four-byte groups from the last), then ll descending (stable)
    int c4 = 0;
    if (sorted && K) {
        for (int i = 0; i < 2; ++i)
            if ((rc = S.take(perm[i], (size_t)K)) || (rc = S.take(key[i], (size_t)K))) return rc;
        uint32_t* const kk[2] = {key[0].p, key[1].p};
        uint32_t* const pp[2] = {perm[0].p, perm[1].p};
        Prof            p(c, COLIBRI_K_SCATTER);
        hipLaunchKernelGGL(cooc_iota_kernel, dim3(stream_grid(K)), dim3(kBlock), 0, c->stream, perm[0].p, (uint64_t)K);
        hipLaunchKernelGGL(cmp_keychunk_kernel, dim3(stream_grid(K)), dim3(kBlock), 0, c->stream, kbytes.p, koff.p, kg.p, perm[0].p, (uint32_t)K, kInvalid, key[0].p);
        if ((rc = radix_sort_pairs(c, kk, pp, K, bits_for((uint64_t)maxkey + 1), c4))) return rc;
        for (int ch = (int)((maxkey + 3) / 4) - 1; ch >= 0; --ch) {
            hipLaunchKernelGGL(cmp_keychunk_kernel, dim3(stream_grid(K)), dim3(kBlock), 0, c->stream, kbytes.p, koff.p, kg.p, perm[c4].p, (uint32_t)K, (uint32_t)ch, key[c4].p);
            if ((rc = radix_sort_pairs(c, kk, pp, K, 32, c4))) return rc;
        }
        for (int half = 0; half < 2; ++half) {
            hipLaunchKernelGGL(cmp_valkey_kernel, dim3(stream_grid(K)), dim3(kBlock), 0, c->stream, ll.p, kd.p, perm[c4].p, (uint32_t)K, half, key[c4].p);
            if ((rc = radix_sort_pairs(c, kk, pp, K, 32, c4))) return rc;
        }
    }
    // (e) the rows in output order
    if ((rc = dev_alloc(c, cm.model, (size_t)K + 1)) || (rc = dev_alloc(c, cm.index, (size_t)K + 1)) || (rc = dev_alloc(c, cm.ll, (size_t)K + 1)) ||
        (rc = dev_alloc(c, cm.observed, (size_t)K * nm + 1)) || (rc = dev_alloc(c, cm.gt, (size_t)K * nm + 1)))
        return rc;
    if (K)
        hipLaunchKernelGGL(cmp_emit_kernel, dim3(stream_grid(K)), dim3(kBlock), 0, c->stream, sorted ? (const uint32_t*)perm[c4].p : (const uint32_t*)nullptr, kd.p, kg.p, ll.p,
                           observed.p, tot.p, ntok.p, cat.p, mstart.p, nm, G, (uint32_t)K, cm.model.p, cm.index.p, cm.ll.p, cm.observed.p, cm.gt.p);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    collect_events(c);
    cm.nrows    = K;
    cm.distinct = D;
    cm.scratch  = S.peak;
    cm.valid    = true;
    *nrows      = K;
    return COLIBRI_OK;
}

int colibri_compare_fetch(colibri_ctx* c, uint32_t* model, uint32_t* index, double* ll, uint32_t* observed, uint32_t* group_totals) {
    if (!c) return COLIBRI_ERR_ARG;
    auto& cm = c->cm;
    if (!cm.valid) return fail(c, COLIBRI_ERR_STATE, "colibri_compare first");
    const uint64_t K = cm.nrows, N = cm.nmodels;
    if (!K) return COLIBRI_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    if (model) HIP_TRY(c, hipMemcpyAsync(model, cm.model.p, sizeof(uint32_t) * K, hipMemcpyDeviceToHost, c->stream));
    if (index) HIP_TRY(c, hipMemcpyAsync(index, cm.index.p, sizeof(uint32_t) * K, hipMemcpyDeviceToHost, c->stream));
    if (ll) HIP_TRY(c, hipMemcpyAsync(ll, cm.ll.p, sizeof(double) * K, hipMemcpyDeviceToHost, c->stream));
    if (observed) HIP_TRY(c, hipMemcpyAsync(observed, cm.observed.p, sizeof(uint32_t) * K * N, hipMemcpyDeviceToHost, c->stream));
    if (group_totals) HIP_TRY(c, hipMemcpyAsync(group_totals, cm.gt.p, sizeof(uint32_t) * K * N, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return COLIBRI_OK;
}

int colibri_compare_info(const colibri_ctx* c, uint64_t* distinct, uint64_t* scratch_bytes) {
    if (!c) return COLIBRI_ERR_ARG;
    if (distinct) *distinct = c->cm.distinct;
    if (scratch_bytes) *scratch_bytes = c->cm.scratch;
    return COLIBRI_OK;
}
