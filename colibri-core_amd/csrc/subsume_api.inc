// subsume_api.inc — part of colibri_hip.hip (included there, inside its extern "C" block, after query_api.inc): the two subsumption prunes of a
// finished model (colibri-patternmodeller -p / --prunesubsumed; kernels and the specification in subsume.hpp). Only the keys are read: counts
// and references are the caller's, who compacts its arrays by the flags. No corpus is needed.

// the device pipeline on a model's keys in HBM, np == 0 included
static int subsume_core(colibri_ctx* c, const ModelView& V, int prunenonsubsumed, int prunesubsumed, int maxlength, uint64_t* nkept) {
    auto&          sb = c->sb;
    const uint32_t np = V.np;
    int            rc;
    DevScratch     S{c};
    sb.np = np;
    if ((rc = dev_alloc(c, sb.keep, np))) return rc;
    if (np == 0) {
        sb.valid = true;
        return COLIBRI_OK;
    }
    const uint64_t hmask = env_hash_mask("COLIBRI_SUBSUME_HASH_BITS");  // (tests: a hash of a few bits, so that the byte check decides identity)
    // one word buffer: cooc_info_kernel's info[4], then per length the histogram, the alive counts and the scatter's cursors, then per level the
    // alive markers of pass 1 and of pass 2
    constexpr uint32_t L = kSubsumeLengths, kHist = 4, kAlive = kHist + L, kCursor = kAlive + L, kMark1 = kCursor + L, kMark2 = kMark1 + L, kWords = kMark2 + L;
    DevBuf<uint8_t>            ntok;
    DevBuf<uint32_t>           pmask, words, list, mark;
    DevBuf<unsigned long long> start, pruned;
    DevBuf<CSlot>              table;
    if ((rc = S.take(ntok, np)) || (rc = S.take(pmask, np)) || (rc = S.take(words, kWords)) || (rc = S.take(start, L)) || (rc = S.take(pruned, 2 * L))) return rc;
    uint32_t hw[kHist + L] = {0xFFFFFFFFu};
    HIP_TRY(c, hipMemsetAsync(words.p, 0, sizeof(uint32_t) * kWords, c->stream));
    HIP_TRY(c, hipMemsetAsync(words.p, 0xFF, sizeof(uint32_t), c->stream));
    HIP_TRY(c, hipMemsetAsync(pruned.p, 0, sizeof(unsigned long long) * 2 * L, c->stream));
    hipLaunchKernelGGL(cooc_info_kernel, dim3(stream_grid(np)), dim3(kBlock), 0, c->stream, V.kbytes, V.koff, np, ntok.p, pmask.p, words.p);
    hipLaunchKernelGGL(subsume_hist_kernel, dim3(stream_grid(np)), dim3(kBlock), 0, c->stream, ntok.p, np, words.p + kHist);
    if ((rc = scan_u32(c, words.p + kHist, L, start.p, nullptr))) return rc;
    HIP_TRY(c, hipMemcpyAsync(words.p + kAlive, words.p + kHist, sizeof(uint32_t) * L, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(hw, words.p, sizeof hw, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // the one look at the model ahead of the ladder: its categories and its lengths
    HIP_TRY(c, hipGetLastError());
    S.drop(pmask);
    if (hw[3] & 4u) return fail(c, COLIBRI_ERR_UNSUPPORTED, "subsume: the model holds a flexgram (a subsumption prune of flexgrams is not on the accelerated path)");
    const uint32_t* hist = hw + kHist;
    const uint32_t  maxtok = hw[1];
    const uint32_t  top1 = (uint32_t)std::min<int64_t>(std::min(prunenonsubsumed, maxlength), maxtok);  // (above the longest pattern every level's M is empty)
    const uint32_t  top2 = (uint32_t)std::min<int64_t>(std::min(prunesubsumed, maxlength), maxtok);
    if (std::max(top1, top2) > (uint32_t)COLIBRI_MAX_ORDER)
        return fail(c, COLIBRI_ERR_OVERFLOW, "subsume: levels up to %u tokens (per-length counts are kept up to %d)", std::max(top1, top2), COLIBRI_MAX_ORDER);
    const uint64_t cap64 = 2ull * np + 1024;
    if (cap64 >= 0xFFFFFFF0ull) return fail(c, COLIBRI_ERR_OVERFLOW, "subsume: %u patterns exceed the key table's 32-bit slots", np);
    const uint32_t cap = (uint32_t)cap64;
    uint64_t       hstart[L + 1];
    hstart[0] = 0;
    for (uint32_t t = 0; t < L; ++t) hstart[t + 1] = hstart[t] + hist[t];
    HIP_TRY(c, hipMemsetAsync(sb.keep.p, 1, np, c->stream));
    if (std::max(top1, top2) >= 2) {
        if ((rc = S.take(list, np)) || (rc = S.take(mark, np)) || (rc = S.take(table, (size_t)cap64))) return rc;
        HIP_TRY(c, hipMemsetAsync(mark.p, 0, sizeof(uint32_t) * np, c->stream));
        Prof prof(c, COLIBRI_K_COUNT);
        hipLaunchKernelGGL(subsume_scatter_kernel, dim3(stream_grid(np)), dim3(kBlock), 0, c->stream, ntok.p, np, start.p, words.p + kCursor, list.p);
        hipLaunchKernelGGL(constraint_clear_kernel, dim3(stream_grid(cap)), dim3(kBlock), 0, c->stream, table.p, cap);
        hipLaunchKernelGGL(constraint_insert_kernel, dim3(stream_grid(np)), dim3(kBlock), 0, c->stream, V.kbytes, V.koff, np, table.p, cap, hmask);
        // level n of a pass: the n-grams mark, the (n-1)-grams are swept. A length the model never had: no launch (its M is empty / nothing to sweep).
        auto level = [&](uint32_t n, bool pass2) {
            if (hist[n] == 0) return;
            const uint32_t tag = pass2 ? (kSubsumePass2 | n) : n;
            hipLaunchKernelGGL(subsume_mark_kernel, dim3(stream_grid(hist[n])), dim3(kBlock), 0, c->stream, list.p + hstart[n], hist[n], sb.keep.p, V.kbytes, V.koff, table.p, cap, hmask, tag,
                               mark.p, words.p + (pass2 ? kMark2 : kMark1) + n);
            if (hist[n - 1] == 0) return;
            hipLaunchKernelGGL(subsume_sweep_kernel, dim3(stream_grid(hist[n - 1])), dim3(kBlock), 0, c->stream, list.p + hstart[n - 1], hist[n - 1], sb.keep.p, mark.p, tag, (int)pass2,
                               pass2 ? (const uint32_t*)nullptr : words.p + kAlive + n, words.p + kAlive + (n - 1), pruned.p + (pass2 ? L : 0u) + (n - 1));
        };
        for (uint32_t n = top1; n >= 2; --n) level(n, false);
        for (uint32_t n = 2; n <= top2; ++n) level(n, true);
    }
    unsigned long long hpruned[2 * L];
    uint32_t           hmarkers[2 * L];
    HIP_TRY(c, hipMemcpyAsync(hpruned, pruned.p, sizeof hpruned, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(hmarkers, words.p + kMark1, sizeof hmarkers, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    collect_events(c);
    uint64_t gone = 0;
    for (uint32_t t = 0; t < (uint32_t)COLIBRI_MAX_ORDER; ++t) {
        sb.pruned_non[t] = hpruned[t];
        sb.pruned_sub[t] = hpruned[L + t];
        gone += hpruned[t] + hpruned[L + t];
    }
    for (uint32_t k = 0; k < 2 * L; ++k) {
        sb.levels += hmarkers[k] != 0;
        sb.probes += 2ull * hmarkers[k];
    }
    sb.scratch = S.peak;
    sb.valid   = true;
    *nkept     = np - gone;
    return COLIBRI_OK;
}

static int subsume_begin(colibri_ctx* c, int prunenonsubsumed, int prunesubsumed, int maxlength, uint64_t* nkept) {
    if (!c || !nkept) return COLIBRI_ERR_ARG;
    auto& sb = c->sb;
    sb.valid = false;
    sb.np    = 0;
    sb.levels = sb.probes = sb.scratch = 0;
    std::fill(std::begin(sb.pruned_non), std::end(sb.pruned_non), 0);
    std::fill(std::begin(sb.pruned_sub), std::end(sb.pruned_sub), 0);
    *nkept = 0;
    if (prunenonsubsumed < 0 || prunesubsumed < 0 || maxlength < 0)
        return fail(c, COLIBRI_ERR_ARG, "subsume: PRUNENONSUBSUMED %d, PRUNESUBSUMED %d, MAXLENGTH %d: none may be negative", prunenonsubsumed, prunesubsumed, maxlength);
    HIP_TRY(c, hipSetDevice(c->device));
    return COLIBRI_OK;
}

int colibri_subsume(colibri_ctx* c, const uint64_t* key_off, const uint8_t* key_bytes, uint64_t npatterns, int prunenonsubsumed, int prunesubsumed, int maxlength, uint64_t* nkept) {
    int rc = subsume_begin(c, prunenonsubsumed, prunesubsumed, maxlength, nkept);
    if (rc) return rc;
    ModelView V;
    if ((rc = model_upload(c, "subsume", key_off, key_bytes, nullptr, nullptr, nullptr, nullptr, npatterns, 0, V))) return rc;
    return subsume_core(c, V, prunenonsubsumed, prunesubsumed, maxlength, nkept);
}

// the same on the model of the last colibri_train of this context, indexed or not, where it lies in HBM: the flags are in export order
int colibri_subsume_resident(colibri_ctx* c, int prunenonsubsumed, int prunesubsumed, int maxlength, uint64_t* npatterns, uint64_t* nkept) {
    if (!npatterns) return COLIBRI_ERR_ARG;
    *npatterns = 0;
    int rc = subsume_begin(c, prunenonsubsumed, prunesubsumed, maxlength, nkept);
    if (rc) return rc;
    ModelView V;
    if ((rc = model_resident(c, "colibri_subsume_resident", false, V))) return rc;
    if ((rc = subsume_core(c, V, prunenonsubsumed, prunesubsumed, maxlength, nkept))) return rc;
    *npatterns = V.np;
    return COLIBRI_OK;
}

int colibri_subsume_fetch(colibri_ctx* c, uint8_t* keep, uint64_t* pruned_non, uint64_t* pruned_sub) {
    if (!c) return COLIBRI_ERR_ARG;
    auto& sb = c->sb;
    if (!sb.valid) return fail(c, COLIBRI_ERR_STATE, "colibri_subsume / colibri_subsume_resident first");
    HIP_TRY(c, hipSetDevice(c->device));
    if (keep && sb.np) {
        HIP_TRY(c, hipMemcpyAsync(keep, sb.keep.p, sb.np, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    if (pruned_non) std::copy(std::begin(sb.pruned_non), std::end(sb.pruned_non), pruned_non);
    if (pruned_sub) std::copy(std::begin(sb.pruned_sub), std::end(sb.pruned_sub), pruned_sub);
    return COLIBRI_OK;
}

int colibri_subsume_info(const colibri_ctx* c, uint64_t* levels, uint64_t* probes, uint64_t* scratch_bytes) {
    if (!c) return COLIBRI_ERR_ARG;
    if (levels) *levels = c->sb.levels;
    if (probes) *probes = c->sb.probes;
    if (scratch_bytes) *scratch_bytes = c->sb.scratch;
    return COLIBRI_OK;
}
