// ngrams_api.inc — part of colibri_hip.hip (included there, inside its extern "C" block, after modelskip_api.inc): n-gram extraction
// (colibri-extractngrams; kernels and the specification in ngrams.hpp).

int colibri_ngrams(colibri_ctx* c, uint32_t n, colibri_decode_sink sink, void* user, uint64_t* outbytes, uint64_t* nngrams) {
    if (!c) return COLIBRI_ERR_ARG;
    if (outbytes) *outbytes = 0;
    if (nngrams) *nngrams = 0;
    if (n == 0) return fail(c, COLIBRI_ERR_ARG, "ngrams: n must be at least 1");
    if (!sink) return fail(c, COLIBRI_ERR_ARG, "ngrams: no sink");
    auto& d = c->dc;  // (the corpus' facts)
    auto& g = c->ng;
    if (!d.ready) return fail(c, COLIBRI_ERR_STATE, "ngrams: no corpus uploaded by colibri_decode_upload");
    if (!c->pr.table) return fail(c, COLIBRI_ERR_STATE, "ngrams: no word table installed by colibri_print_classes");
    if (d.v1) return fail(c, COLIBRI_ERR_UNSUPPORTED, "ngrams: the corpus was uploaded as version 1 data; only version 2 data has n-grams to extract");
    g.windows = g.staging = g.scratch = 0;
    const uint32_t npos = c->npos;
    if (npos == 0) return COLIBRI_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const PrintTable           tab{c->pr.wordoff.p, c->pr.words.p, c->pr.has.p, c->pr.nids};
    DevScratch                 S{c};
    DevBuf<uint32_t>           wl, flag, gpos, glen, range, bad;
    DevBuf<unsigned long long> P, idx, G, bsum;
    const uint32_t             nb = blocks_for(npos, kBlock * 4);
    int                        rc;
    auto scan = [&](const uint32_t* in, uint32_t m, unsigned long long* out) {  // out[0 .. m] = the exclusive scan of in[0 .. m) and its total
        const uint32_t b = blocks_for(m, kBlock * 4);
        hipLaunchKernelGGL(scan_reduce_kernel, dim3(b), dim3(kBlock), 0, c->stream, in, m, bsum.p);
        hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(kBlock), 0, c->stream, bsum.p, b, out + m);
        hipLaunchKernelGGL(scan_apply_kernel, dim3(b), dim3(kBlock), 0, c->stream, in, m, bsum.p, out);
    };
    if ((rc = S.take(wl, npos)) || (rc = S.take(flag, npos)) || (rc = S.take(P, (size_t)npos + 1)) || (rc = S.take(idx, (size_t)npos + 1)) || (rc = S.take(bsum, nb)) ||
        (rc = S.take(range, 2)) || (rc = S.take(bad, 1)))
        return rc;
    HIP_TRY(c, hipMemsetAsync(bad.p, 0, sizeof(uint32_t), c->stream));
    hipLaunchKernelGGL(ngrams_word_kernel, dim3(stream_grid(npos)), dim3(kBlock), 0, c->stream, c->cls.p, c->delimpos.p, c->ndelim, npos, (unsigned long long)n, tab, wl.p, flag.p, bad.p);
    scan(wl.p, npos, P.p);
    scan(flag.p, npos, idx.p);
    unsigned long long m = 0;
    HIP_TRY(c, hipMemcpyAsync(&m, idx.p + npos, sizeof m, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    g.scratch = S.peak;
    if (m == 0) return COLIBRI_OK;  // (n above every line)
    if ((rc = S.take(gpos, m)) || (rc = S.take(glen, m)) || (rc = S.take(G, (size_t)m + 1))) return rc;
    hipLaunchKernelGGL(ngrams_gather_kernel, dim3(stream_grid(npos)), dim3(kBlock), 0, c->stream, wl.p, flag.p, idx.p, P.p, npos, n, gpos.p, glen.p, bad.p);
    scan(glen.p, (uint32_t)m, G.p);
    unsigned long long total = 0;
    uint32_t           hbad  = 0;
    HIP_TRY(c, hipMemcpyAsync(&total, G.p + m, sizeof total, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(&hbad, bad.p, sizeof hbad, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    g.scratch = S.peak;
    S.drop(wl);
    S.drop(flag);
    S.drop(P);
    S.drop(idx);
    S.drop(glen);
    S.drop(bsum);
    if (hbad & kNgramsBadRow)
        return fail(c, COLIBRI_ERR_OVERFLOW, "ngrams: a word or an n-gram's text takes %u bytes (4 MiB) or more: the scans add up to 1024 of them in 32 bits", kNgramsMaxRow);
    rc = pump_windows(
        c, S, "ngrams", "call", "COLIBRI_NGRAMS_WINDOW_BYTES", kNgramsWindowBytes, total, sink, user,
        [&](unsigned long long W0, unsigned long long W1, uint8_t* stage) {
            hipLaunchKernelGGL(decode_range_kernel, dim3(1), dim3(kWave), 0, c->stream, G.p, (uint32_t)m, W0, W1, range.p);
            hipLaunchKernelGGL(ngrams_lane_kernel, dim3(stream_grid(std::min<uint64_t>(m, W1 - W0 + 1))), dim3(kBlock), 0, c->stream, c->cls.p, gpos.p, G.p, n, tab, range.p, W0, W1, stage);
        },
        &g.windows, &g.staging);
    g.scratch = S.peak;
    if (rc) return rc;
    if (outbytes) *outbytes = total;
    if (nngrams) *nngrams = m;
    return COLIBRI_OK;
}

int colibri_ngrams_info(const colibri_ctx* c, uint64_t* windows, uint64_t* staging_bytes, uint64_t* scratch_bytes) {
    if (!c) return COLIBRI_ERR_ARG;
    if (windows) *windows = c->ng.windows;
    if (staging_bytes) *staging_bytes = c->ng.staging;
    if (scratch_bytes) *scratch_bytes = c->ng.scratch;
    return COLIBRI_OK;
}
