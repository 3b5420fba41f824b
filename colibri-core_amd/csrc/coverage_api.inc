// coverage_api.inc — part of colibri_hip.hip (included there, inside its extern "C" block, after decode_api.inc): the coverage report of a
// pattern model (colibri-patternmodeller -R / -r; kernels and the specification in coverage.hpp).
extern "C++" {
namespace {
// group -> bitmap: a group without members gets none; a group that holds as many patterns as a group containing it is that group and shares its
// bitmap. (0, 0) contains (c, 0) and (0, n); those two contain (c, n). per_size = false: only the all-sizes groups get one.
uint32_t cov_assign_slots(const uint64_t* members, uint32_t G, bool per_size, std::vector<uint32_t>& slot) {
    slot.assign(4 * (size_t)G, kCovNoSlot);
    uint32_t nb = 0;
    if (!members[0]) return 0;
    slot[0] = nb++;
    for (uint32_t c = 1; c < 4; ++c)
        if (members[c * G]) slot[c * G] = members[c * G] == members[0] ? slot[0] : nb++;
    if (!per_size) return nb;
    for (uint32_t n = 1; n < G; ++n) {
        if (!members[n]) continue;
        slot[n] = members[n] == members[0] ? slot[0] : nb++;
        for (uint32_t c = 1; c < 4; ++c) {
            const uint64_t m = members[c * G + n];
            if (m) slot[c * G + n] = m == members[n] ? slot[n] : m == members[c * G] ? slot[c * G] : nb++;
        }
    }
    return nb;
}
}  // namespace
}  // extern "C++"

// the device pipeline on a model in HBM, indexed or not
static int cov_core(colibri_ctx* c, const ModelView& V, int flags, uint64_t* ngroups_n) {
    const uint32_t np    = V.np;
    const uint64_t nrefs = V.nrefs;
    auto&          cv = c->cv;
    int            rc;
    DevScratch     S{c};
    const uint64_t budget = env_u64("COLIBRI_COV_BUDGET", kCovBudgetBytes);
    const uint32_t slice  = (uint32_t)std::max<uint64_t>(std::min<uint64_t>(env_u64("COLIBRI_COV_SLICE", kCovSlice), 1u << 20), (nrefs >> 30) + 1);  // (the grid stays under 2^30 blocks)
    const char*    te     = getenv("COLIBRI_COV_TEST");
    const bool     test   = !(te && te[0] == '0');  // (measurements: 0 = every touched word gets its atomicOr, set already or not)
    DevBuf<uint16_t>           ntok;
    DevBuf<uint8_t>            cat;
    DevBuf<unsigned long long> info, grp, sums, base;
    DevBuf<uint32_t>           slot, bits, rinfo, extent;
    // (a) per pattern: tokens, category; the model's most tokens and largest class id
    if ((rc = S.take(ntok, np)) || (rc = S.take(cat, np)) || (rc = S.take(info, 2))) return rc;
    HIP_TRY(c, hipMemsetAsync(info.p, 0, 2 * sizeof(unsigned long long), c->stream));
    hipLaunchKernelGGL(cov_info_kernel, dim3(stream_grid(np)), dim3(kBlock), 0, c->stream, V.kbytes, V.koff, np, ntok.p, cat.p, info.p);
    unsigned long long hinfo[2];
    HIP_TRY(c, hipMemcpyAsync(hinfo, info.p, sizeof hinfo, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    if (hinfo[0] > 0xFFFFull) return fail(c, COLIBRI_ERR_OVERFLOW, "coverage: a pattern of %llu tokens (at most 65535)", hinfo[0]);
    const uint32_t G  = (uint32_t)hinfo[0] + 1;
    const size_t   NG = 4 * (size_t)G;
    // (b) patterns / counts / members per group
    if ((rc = S.take(grp, 3 * NG))) return rc;
    HIP_TRY(c, hipMemsetAsync(grp.p, 0, sizeof(unsigned long long) * 3 * NG, c->stream));
    {
        const bool lds = 3 * NG * sizeof(unsigned long long) <= 32768;
        hipLaunchKernelGGL(cov_group_kernel, dim3(stream_grid(np)), dim3(kBlock), lds ? 3 * NG * sizeof(unsigned long long) : 0, c->stream, ntok.p, cat.p, V.cnt, V.roff, np, G, (int)lds,
                           grp.p);
    }
    std::vector<uint64_t> hgrp(3 * NG);
    HIP_TRY(c, hipMemcpyAsync(hgrp.data(), grp.p, sizeof(uint64_t) * 3 * NG, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    const uint64_t* members = hgrp.data() + 2 * NG;
    cv.res.assign(4 * NG, 0);
    std::copy(hgrp.begin(), hgrp.begin() + 2 * NG, cv.res.begin());
    std::vector<uint32_t> hslot;
    std::vector<uint64_t> hsums;
    // (c) word types: one class bitmap per distinct group
    {
        const uint32_t nb = cov_assign_slots(members, G, true, hslot);
        const uint64_t CW = hinfo[1] / 32 + 1;  // words of maxclass + 1 bits
        if (hinfo[1] == ~0ull || nb > 65535 || CW > budget / 4 / std::max(nb, 1u))  // (one grid row per bitmap)
            return fail(c, COLIBRI_ERR_OVERFLOW, "coverage: %u class bitmaps up to class %llu exceed the scratch budget of %llu bytes (COLIBRI_COV_BUDGET)", nb, hinfo[1],
                        (unsigned long long)budget);
        if ((rc = S.take(slot, NG)) || (rc = S.take(bits, (size_t)(nb * CW))) || (rc = S.take(sums, nb))) return rc;
        HIP_TRY(c, hipMemcpyAsync(slot.p, hslot.data(), sizeof(uint32_t) * NG, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemsetAsync(bits.p, 0, sizeof(uint32_t) * nb * CW, c->stream));
        HIP_TRY(c, hipMemsetAsync(sums.p, 0, sizeof(unsigned long long) * nb, c->stream));
        hipLaunchKernelGGL(cov_types_kernel, dim3(stream_grid(np)), dim3(kBlock), 0, c->stream, V.kbytes, V.koff, ntok.p, cat.p, np, G, slot.p, (unsigned long long)CW, bits.p);
        hipLaunchKernelGGL(cov_popc_kernel, dim3(stream_grid(CW), nb), dim3(kBlock), 0, c->stream, bits.p, (unsigned long long)CW, sums.p);
        hsums.assign(nb, 0);
        HIP_TRY(c, hipMemcpyAsync(hsums.data(), sums.p, sizeof(uint64_t) * nb, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));  // (hslot is free again)
        HIP_TRY(c, hipGetLastError());
        for (size_t g = 0; g < NG; ++g)
            if (hslot[g] != kCovNoSlot) cv.res[2 * NG + g] = hsums[hslot[g]];
        cv.bitmap_bytes = sizeof(uint32_t) * nb * CW;
        S.drop(bits);
        S.drop(sums);
    }
    // (d) covered tokens: sentence range, extents, bases, one position bitmap per distinct group
    if (V.roff && nrefs && !(flags & COLIBRI_COV_NO_TOKENS)) {
        const bool per_size = (flags & COLIBRI_COV_PER_SIZE) != 0;
        if ((rc = S.take(rinfo, 2))) return rc;
        const uint32_t r0[2] = {0xFFFFFFFFu, 0u};
        HIP_TRY(c, hipMemcpyAsync(rinfo.p, r0, sizeof r0, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(cov_range_kernel, dim3(stream_grid(nrefs)), dim3(kBlock), 0, c->stream, V.rs, nrefs, rinfo.p);
        uint32_t hr[2];
        HIP_TRY(c, hipMemcpyAsync(hr, rinfo.p, sizeof hr, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        HIP_TRY(c, hipGetLastError());
        const uint64_t nsent = (uint64_t)hr[1] - hr[0] + 1;
        if (nsent > budget / 12 || nsent >= 0xFFFFFFF0ull)
            return fail(c, COLIBRI_ERR_OVERFLOW, "coverage: the sentence range %u..%u exceeds the scratch budget of %llu bytes (COLIBRI_COV_BUDGET)", hr[0], hr[1],
                        (unsigned long long)budget);
        if ((rc = S.take(extent, (size_t)nsent + 1)) || (rc = S.take(base, (size_t)nsent + 1))) return rc;
        HIP_TRY(c, hipMemsetAsync(extent.p, 0, sizeof(uint32_t) * (nsent + 1), c->stream));
        const uint32_t nblk = blocks_for(nrefs, slice);
        hipLaunchKernelGGL(cov_extent_kernel, dim3(nblk), dim3(kBlock), 0, c->stream, V.roff, V.rs, V.rt, ntok.p, np, nrefs, slice, hr[0], extent.p);
        unsigned long long P = 0;
        if ((rc = scan_u32(c, extent.p, (uint32_t)nsent + 1, base.p, &P))) return rc;
        S.drop(extent);
        const uint32_t nb = cov_assign_slots(members, G, per_size, hslot);
        const uint64_t W  = P / 32 + 1;
        if (nb > 65535 || W > (budget - nsent * 12) / 4 / std::max(nb, 1u))
            return fail(c, COLIBRI_ERR_OVERFLOW, "coverage: %u bitmaps of %llu positions exceed the scratch budget of %llu bytes (COLIBRI_COV_BUDGET)", nb, P,
                        (unsigned long long)budget);
        if ((rc = S.take(bits, (size_t)(nb * W))) || (rc = S.take(sums, nb))) return rc;
        HIP_TRY(c, hipMemcpyAsync(slot.p, hslot.data(), sizeof(uint32_t) * NG, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemsetAsync(bits.p, 0, sizeof(uint32_t) * nb * W, c->stream));
        HIP_TRY(c, hipMemsetAsync(sums.p, 0, sizeof(unsigned long long) * nb, c->stream));
        if (test)
            hipLaunchKernelGGL(cov_mark_kernel<true>, dim3(nblk), dim3(kBlock), 0, c->stream, V.roff, V.rs, V.rt, ntok.p, cat.p, np, nrefs, slice, hr[0], base.p, G, slot.p,
                               (unsigned long long)W, bits.p);
        else
            hipLaunchKernelGGL(cov_mark_kernel<false>, dim3(nblk), dim3(kBlock), 0, c->stream, V.roff, V.rs, V.rt, ntok.p, cat.p, np, nrefs, slice, hr[0], base.p, G, slot.p,
                               (unsigned long long)W, bits.p);
        hipLaunchKernelGGL(cov_popc_kernel, dim3(stream_grid(W), nb), dim3(kBlock), 0, c->stream, bits.p, (unsigned long long)W, sums.p);
        hsums.assign(nb, 0);
        HIP_TRY(c, hipMemcpyAsync(hsums.data(), sums.p, sizeof(uint64_t) * nb, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        HIP_TRY(c, hipGetLastError());
        for (size_t g = 0; g < NG; ++g)
            if (hslot[g] != kCovNoSlot) cv.res[3 * NG + g] = hsums[hslot[g]];
        cv.marked = nrefs;
        cv.bitmap_bytes += sizeof(uint32_t) * nb * W;
    }
    cv.G       = G;
    cv.scratch = S.peak;
    cv.valid   = true;
    *ngroups_n = G;
    return COLIBRI_OK;
}

static int coverage_begin(colibri_ctx* c, int flags, uint64_t* ngroups_n) {
    if (!c || !ngroups_n || (flags & ~(COLIBRI_COV_PER_SIZE | COLIBRI_COV_NO_TOKENS))) return COLIBRI_ERR_ARG;
    auto& cv = c->cv;
    cv.valid = false;
    cv.res.clear();
    cv.G = 0;
    cv.marked = cv.bitmap_bytes = cv.scratch = 0;
    *ngroups_n = 0;
    return COLIBRI_OK;
}

int colibri_coverage(colibri_ctx* c, const uint64_t* key_off, const uint8_t* key_bytes, const uint32_t* counts, const uint64_t* ref_off, const uint32_t* ref_sentence,
                     const uint16_t* ref_token, uint64_t npatterns, int flags, uint64_t* ngroups_n) {
    int rc = coverage_begin(c, flags, ngroups_n);
    if (rc) return rc;
    if (npatterns == 0) {
        c->cv.valid = true;
        return COLIBRI_OK;
    }
    ModelView V;
    if ((rc = model_upload(c, "coverage", key_off, key_bytes, counts, ref_off, ref_sentence, ref_token, npatterns, kModelCounts | kModelOffsets | kModelRefs, V))) return rc;
    return cov_core(c, V, flags, ngroups_n);
}

// the indexed model of the last colibri_train of this context, still resident in HBM (the corpus is not read)
int colibri_coverage_resident(colibri_ctx* c, int flags, uint64_t* ngroups_n) {
    int rc = coverage_begin(c, flags, ngroups_n);
    if (rc) return rc;
    ModelView V;
    if ((rc = model_resident(c, "colibri_coverage_resident", true, V))) return rc;
    if (V.np == 0) {
        c->cv.valid = true;
        return COLIBRI_OK;
    }
    return cov_core(c, V, flags, ngroups_n);
}

int colibri_coverage_fetch(colibri_ctx* c, uint64_t* patterns, uint64_t* counts, uint64_t* types, uint64_t* tokens) {
    if (!c) return COLIBRI_ERR_ARG;
    const auto& cv = c->cv;
    if (!cv.valid) return fail(c, COLIBRI_ERR_STATE, "colibri_coverage / colibri_coverage_resident first");
    const size_t NG        = 4 * (size_t)cv.G;
    uint64_t*    out[4]    = {patterns, counts, types, tokens};
    for (int k = 0; k < 4; ++k)
        if (out[k] && NG) std::copy(cv.res.begin() + k * NG, cv.res.begin() + (k + 1) * NG, out[k]);
    return COLIBRI_OK;
}

int colibri_coverage_info(const colibri_ctx* c, uint64_t* references, uint64_t* bitmap_bytes, uint64_t* scratch_bytes) {
    if (!c) return COLIBRI_ERR_ARG;
    if (references) *references = c->cv.marked;
    if (bitmap_bytes) *bitmap_bytes = c->cv.bitmap_bytes;
    if (scratch_bytes) *scratch_bytes = c->cv.scratch;
    return COLIBRI_OK;
}
