// cooc_api.inc — part of colibri_hip.hip (included there, inside its extern "C" block): sentence co-occurrence of an indexed model
// (colibri-patternmodeller -C / -Y; kernels and the specification in cooc.hpp).
extern "C++" {
namespace {
// ---- the reverse-index stage, shared by cooc_core and the reverse index of its own (rindex_api.inc) ---------------------------------------------
struct RevLayers {
    int      minn = 0, maxn = 0;
    uint32_t maxkey = 0;
    std::vector<std::pair<int, uint32_t>> layers;  // (length, gap mask): every length, then every (length, mask) a skipgram of the model has (length >= 3)
    uint32_t ngram_layers() const { return (uint32_t)(maxn - minn + 1); }
};
// from cooc_info_kernel's results (info[0..3], ntok, pmask): the model's lengths and its layers. A flexgram in the model is refused
// (COLIBRI_ERR_UNSUPPORTED), a skipgram of more than kMaskedMaxTokens tokens with `toolong`.
int rev_layers(colibri_ctx* c, const char* what, int toolong, const uint8_t* ntok, const uint32_t* pmask, const uint32_t* info, uint32_t np, RevLayers& R) {
    uint32_t hinfo[4];
    HIP_TRY(c, hipMemcpyAsync(hinfo, info, sizeof hinfo, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    if (hinfo[3] & 4) return fail(c, COLIBRI_ERR_UNSUPPORTED, "%s: the model holds flexgrams (the reference matches them by flexgramsize, outside this build)", what);
    R.minn   = (int)hinfo[0];
    R.maxn   = (int)hinfo[1];
    R.maxkey = hinfo[2];
    R.layers.clear();
    for (int n = R.minn; n <= R.maxn; ++n) R.layers.push_back({n, 0u});
    if (hinfo[3] & 2) {
        std::vector<uint8_t>  hn(np);
        std::vector<uint32_t> hm(np);
        HIP_TRY(c, hipMemcpyAsync(hn.data(), ntok, np, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(hm.data(), pmask, sizeof(uint32_t) * np, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        std::vector<std::pair<int, uint32_t>> sk;
        for (uint32_t p = 0; p < np; ++p)
            if (hm[p] && hn[p] >= 3) sk.push_back({(int)hn[p], hm[p]});
        std::sort(sk.begin(), sk.end());
        sk.erase(std::unique(sk.begin(), sk.end()), sk.end());
        for (const auto& s : sk) {
            if (s.first > kMaskedMaxTokens) return fail(c, toolong, "%s: skipgrams of more than %d tokens", what, kMaskedMaxTokens);
            R.layers.push_back(s);
        }
    }
    return COLIBRI_OK;
}
// the model's keys into the table; the per-position sentence remainders of the corpus, once per upload
int rev_table(colibri_ctx* c, const uint8_t* kbytes, const unsigned long long* koff, uint32_t np, CSlot* table, uint32_t cap) {
    int rc;
    hipLaunchKernelGGL(constraint_clear_kernel, dim3(stream_grid(cap)), dim3(kBlock), 0, c->stream, table, cap);
    hipLaunchKernelGGL(constraint_insert_kernel, dim3(stream_grid(np)), dim3(kBlock), 0, c->stream, kbytes, koff, np, table, cap, ~0ull);
    if (!c->cs.rem_valid) {
        if ((rc = dev_alloc(c, c->cs.rem, (size_t)c->npos + 1))) return rc;
        hipLaunchKernelGGL(sentence_rem_kernel, dim3(stream_grid(c->npos)), dim3(kBlock), 0, c->stream, c->delimpos.p, c->ndelim, c->npos, c->cs.rem.p);
        c->cs.rem_valid = true;
    }
    return COLIBRI_OK;
}
// memb[l * stride + j] = the pattern number of layer l's window at position p0 + j, j < n (kInvalid: none). Runs of n-gram layers of consecutive
// lengths share a probe pass, kProbeLengths at a time; a window stops at its sentence's end (rem), so the range may be cut anywhere. gate: n + 1
// words (only read with masked layers).
void rev_probe(colibri_ctx* c, const uint8_t* kbytes, const unsigned long long* koff, const std::vector<std::pair<int, uint32_t>>& layers, const CSlot* table, uint32_t cap,
               uint32_t p0, uint32_t n, uint32_t* memb, size_t stride, uint32_t* gate) {
    const uint32_t L = (uint32_t)layers.size();
    for (uint32_t l = 0; l < L;) {
        if (layers[l].second == 0) {
            uint32_t len = 1;
            while (l + len < L && len < (uint32_t)kProbeLengths && layers[l + len].second == 0 && layers[l + len].first == layers[l].first + (int)len) ++len;
            hipLaunchKernelGGL(constraint_probe_kernel<false>, dim3(stream_grid(n)), dim3(kBlock), 0, c->stream, c->bytes.p, c->tokstart.p + p0, c->cs.rem.p + p0, table, cap, kbytes, koff,
                               n, layers[l].first, (int)len, memb + (size_t)l * stride, stride, (const uint32_t*)nullptr, ~0ull);
            l += len;
        } else {
            hipLaunchKernelGGL(cooc_gate_kernel, dim3(stream_grid(n)), dim3(kBlock), 0, c->stream, c->cs.rem.p + p0, n, (uint32_t)layers[l].first, gate);
            hipLaunchKernelGGL(constraint_probe_masked_kernel, dim3(stream_grid(n)), dim3(kBlock), 0, c->stream, c->bytes.p, c->tokstart.p + p0, gate, table, cap, kbytes, koff, n,
                               layers[l].first, layers[l].second, memb + (size_t)l * stride);
            ++l;
        }
    }
}
// the skip content (skiprel.hpp) through cooc_core: what the identity step leaves for the pipeline and for the caller
struct SkcHook {
    DevBuf<uint32_t>           cnum, da, dsrc, dlen, dpb;  // per reference: its pair's number; per distinct (A, content) pair: A, the bytes' place, length, model number
    DevBuf<uint8_t>            dbytes;                     // the distinct contents as key bytes
    DevBuf<unsigned long long> doff;
    uint64_t                   nd = 0, rounds = 0, skipped = 0;
    uint32_t                   maxlen = 0;
    colibri_ctx::CoocState     rows;  // (A, pair number, count) in output order
};
int skc_identity(colibri_ctx* c, DevScratch& S, const RelArgs& r, uint64_t nrefs, SkcHook& H);  // skiprel_api.inc
}  // namespace
}  // extern "C++"

// the device pipeline on an indexed model in HBM. rel < 0: sentence co-occurrence into c->co; rel = a RelKind (relations.hpp): that relation into c->rl, with its own event / emit kernels and row order;
// with `skc` (rel = kRelInstances, threshold 0: the B list unfiltered): the skip content into skc->rows — the B side is then the (A, content)
// pairs skc_identity numbers, not patterns
static int cooc_core(colibri_ctx* c, const ModelView& V, uint32_t threshold, int npmi, double npmi_threshold, uint64_t* nrows, int rel = -1, SkcHook* skc = nullptr) {
    const uint32_t np    = V.np;
    const uint64_t nrefs = V.nrefs;
    auto&       co   = rel < 0 ? c->co : skc ? skc->rows : c->rl;
    const char* what = rel < 0 ? "cooc" : skc ? "skipcontent" : "relations";
    const uint32_t bthr = rel == kRelTemplates ? 0u : threshold;  // templates look up B whatever its own count
    int         rc;
    DevScratch  S{c};
    DevBuf<uint8_t>            ntok, bn;
    DevBuf<uint32_t>           pmask, info, cnt, memb, gate, hits, bpos, bid, aid, events, maxev, ka[2], kb[2], head, perm[2], key[2], ra, rb, rc_, keep, rank, cmid, cfirst,
                               clast, carb, carc, mk[2], mp[2], mw, ma, mb, mc;
    DevBuf<unsigned long long> boff, evoff, cstart, cbase, rid, rstart, kofs, bnd;
    DevBuf<CSlot>              table;
    DevBuf<double>             val;
    DevBuf<uint8_t>            layer_n;
    const uint32_t npos = c->npos, ndelim = c->ndelim, nsent = ndelim + 1;  // (the positions after the last delimiter form sentence ndelim, possibly empty)
    const size_t   stride = (size_t)npos + 1;
    // per pattern: tokens, gap mask, category; the model's lengths; occurrence counts (= forward index lengths)
    if ((rc = S.take(ntok, np)) || (rc = S.take(pmask, np)) || (rc = S.take(info, 4)) || (rc = S.take(cnt, np))) return rc;
    const uint32_t info0[4] = {0xFFFFFFFFu, 0u, 0u, 0u};
    HIP_TRY(c, hipMemcpyAsync(info.p, info0, sizeof info0, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(cooc_info_kernel, dim3(stream_grid(np)), dim3(kBlock), 0, c->stream, V.kbytes, V.koff, np, ntok.p, pmask.p, info.p);
    hipLaunchKernelGGL(cooc_count_kernel, dim3(stream_grid(np)), dim3(kBlock), 0, c->stream, V.roff, np, cnt.p);
    RevLayers RL;
    if ((rc = rev_layers(c, what, COLIBRI_ERR_UNSUPPORTED, ntok.p, pmask.p, info.p, np, RL))) return rc;
    const int      maxn   = RL.maxn;
    const uint32_t maxkey = RL.maxkey;
    const auto&    layers = RL.layers;
    const uint32_t L = (uint32_t)layers.size();
    std::vector<uint8_t> hlayer_n(L);
    for (uint32_t l = 0; l < L; ++l) hlayer_n[l] = (uint8_t)layers[l].first;
    // (a) the reverse index: the model's keys in a table, every window of every layer looked up
    const uint64_t cap64 = 2ull * np + 1024;
    if ((rc = S.take(table, (size_t)cap64)) || (rc = S.take(memb, (size_t)L * stride)) || (rc = S.take(layer_n, L))) return rc;
    const uint32_t cap = (uint32_t)cap64;
    HIP_TRY(c, hipMemcpyAsync(layer_n.p, hlayer_n.data(), L, hipMemcpyHostToDevice, c->stream));
    {
        Prof p(c, COLIBRI_K_COUNT);
        if ((rc = rev_table(c, V.kbytes, V.koff, np, table.p, cap))) return rc;
        if (L > RL.ngram_layers() && (rc = S.take(gate, stride))) return rc;
        rev_probe(c, V.kbytes, V.koff, layers, table.p, cap, 0, npos, memb.p, stride, gate.p);
    }
    S.drop(gate);
    S.drop(table);
    // the B list, by position
    unsigned long long EB = 0;
    if ((rc = S.take(hits, stride)) || (rc = S.take(boff, stride))) return rc;
    HIP_TRY(c, hipMemsetAsync(hits.p, 0, sizeof(uint32_t) * stride, c->stream));
    hipLaunchKernelGGL(cooc_hits_kernel, dim3(stream_grid(npos)), dim3(kBlock), 0, c->stream, memb.p, stride, L, npos, cnt.p, bthr, hits.p);
    if ((rc = scan_u32(c, hits.p, npos + 1, boff.p, &EB))) return rc;
    S.drop(hits);
    if ((rc = S.take(bpos, (size_t)EB + 1)) || (rc = S.take(bn, (size_t)EB + 1)) || (rc = S.take(bid, (size_t)EB + 1))) return rc;
    hipLaunchKernelGGL(cooc_bfill_kernel, dim3(stream_grid(npos)), dim3(kBlock), 0, c->stream, memb.p, stride, L, layer_n.p, npos, cnt.p, bthr, boff.p, bpos.p, bn.p, bid.p);
    S.drop(memb);
    // (b) the A side: every reference of the forward index, with its pattern
    if ((rc = S.take(aid, (size_t)nrefs + 1))) return rc;
    hipLaunchKernelGGL(cooc_aocc_kernel, dim3(stream_grid(nrefs)), dim3(kBlock), 0, c->stream, V.roff, np, nrefs, aid.p);
    // (c) pair events per A occurrence; chunks of consecutive references whose events fit the budget (a cut may fall inside a pattern)
    unsigned long long E = 0;
    if ((rc = S.take(events, (size_t)nrefs + 1)) || (rc = S.take(evoff, (size_t)nrefs + 1)) || (rc = S.take(maxev, 1))) return rc;
    HIP_TRY(c, hipMemsetAsync(events.p + nrefs, 0, sizeof(uint32_t), c->stream));
    HIP_TRY(c, hipMemsetAsync(maxev.p, 0, sizeof(uint32_t), c->stream));
    const RelArgs ra_{V.rs, aid.p, V.rt, ntok.p, pmask.p, V.kbytes, V.koff, c->delimpos.p, ndelim, npos, nsent, c->first_sentence, (uint32_t)maxn, boff.p, bpos.p, bn.p, bid.p,
                      c->bytes.p, c->tokstart.p, cnt.p, threshold};
    if (skc && (rc = skc_identity(c, S, ra_, nrefs, *skc))) return rc;
    const uint64_t nids = skc ? std::max<uint64_t>(np, skc->nd) : np;  // the B side's numbers: patterns, or (A, content) pairs
    {
        Prof p(c, COLIBRI_K_EMIT);
        if (skc)
            hipLaunchKernelGGL(skc_events_kernel, dim3(stream_grid(nrefs)), dim3(kBlock), 0, c->stream, skc->cnum.p, nrefs, events.p, maxev.p);
        else if (rel < 0)
            hipLaunchKernelGGL(cooc_events_kernel, dim3(stream_grid(nrefs * kCoocWave)), dim3(kBlock), 0, c->stream, nrefs, nsent, c->first_sentence, V.rs, aid.p, V.rt, ntok.p,
                               c->delimpos.p, ndelim, npos, boff.p, bpos.p, bn.p, events.p, maxev.p);
        else if (rel == kRelSubchildren)
            hipLaunchKernelGGL(rel_events_kernel<kRelSubchildren>, dim3(stream_grid(nrefs)), dim3(kBlock), 0, c->stream, ra_, nrefs, events.p, maxev.p);
        else if (rel == kRelSubparents)
            hipLaunchKernelGGL(rel_events_kernel<kRelSubparents>, dim3(stream_grid(nrefs)), dim3(kBlock), 0, c->stream, ra_, nrefs, events.p, maxev.p);
        else if (rel == kRelLeft)
            hipLaunchKernelGGL(rel_events_kernel<kRelLeft>, dim3(stream_grid(nrefs)), dim3(kBlock), 0, c->stream, ra_, nrefs, events.p, maxev.p);
        else if (rel == kRelInstances)
            hipLaunchKernelGGL(rel_events_kernel<kRelInstances>, dim3(stream_grid(nrefs)), dim3(kBlock), 0, c->stream, ra_, nrefs, events.p, maxev.p);
        else if (rel == kRelTemplates)
            hipLaunchKernelGGL(rel_events_kernel<kRelTemplates>, dim3(stream_grid(nrefs)), dim3(kBlock), 0, c->stream, ra_, nrefs, events.p, maxev.p);
        else
            hipLaunchKernelGGL(rel_events_kernel<kRelRight>, dim3(stream_grid(nrefs)), dim3(kBlock), 0, c->stream, ra_, nrefs, events.p, maxev.p);
    }
    if ((rc = scan_u32(c, events.p, (uint32_t)nrefs + 1, evoff.p, &E))) return rc;
    S.drop(events);
    uint32_t hmaxev = 0;
    HIP_TRY(c, hipMemcpyAsync(&hmaxev, maxev.p, sizeof hmaxev, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const uint64_t budget = env_u64(rel < 0 ? "COLIBRI_COOC_CHUNK" : "COLIBRI_REL_CHUNK", kCoocChunkEvents);  // (tests: many small chunks on a small corpus)
    const uint64_t nch64  = std::max<uint64_t>(1, (E + budget - 1) / budget);
    if (nch64 > 0x7FFFFFFFull) return fail(c, COLIBRI_ERR_OVERFLOW, "%s: %llu chunks", what, (unsigned long long)nch64);
    const uint32_t nchunks = (uint32_t)nch64;
    const uint64_t capev   = std::min<uint64_t>(E, budget + hmaxev) + 1;  // (a chunk ends before the first reference whose events begin past its share)
    if (capev >= 0xFFFFFFF0ull) return fail(c, COLIBRI_ERR_OVERFLOW, "%s: %llu pair events in one chunk", what, (unsigned long long)capev);
    if ((rc = S.take(cstart, (size_t)nchunks + 1)) || (rc = S.take(cbase, (size_t)nchunks + 1)) || (rc = S.take(cmid, (size_t)nchunks + 1)) ||
        (rc = S.take(cfirst, (size_t)nchunks + 1)) || (rc = S.take(clast, (size_t)nchunks + 1)))
        return rc;
    hipLaunchKernelGGL(cooc_chunks_kernel, dim3(stream_grid((uint64_t)nchunks + 1)), dim3(kBlock), 0, c->stream, evoff.p, nrefs, aid.p, budget, nchunks, cstart.p, cbase.p, cmid.p,
                       cfirst.p, clast.p);
    std::vector<unsigned long long> hstart((size_t)nchunks + 1), hbase((size_t)nchunks + 1);
    std::vector<uint32_t>           hmid((size_t)nchunks + 1), hfirst((size_t)nchunks + 1), hlast((size_t)nchunks + 1);
    HIP_TRY(c, hipMemcpyAsync(hstart.data(), cstart.p, sizeof(unsigned long long) * (nchunks + 1), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(hbase.data(), cbase.p, sizeof(unsigned long long) * (nchunks + 1), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(hmid.data(), cmid.p, sizeof(uint32_t) * (nchunks + 1), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(hfirst.data(), cfirst.p, sizeof(uint32_t) * (nchunks + 1), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(hlast.data(), clast.p, sizeof(uint32_t) * (nchunks + 1), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    const uint64_t mcap = 2ull * nids + 2;                // the runs of one pattern: at most one per B, carried + the chunk's
    const uint64_t fcap = std::max<uint64_t>(capev, mcap);  // runs valued at once: a chunk's, or one merged pattern's
    for (int i = 0; i < 2; ++i)
        if ((rc = S.take(ka[i], (size_t)capev)) || (rc = S.take(kb[i], (size_t)capev)) || (rc = S.take(mk[i], (size_t)mcap)) || (rc = S.take(mp[i], (size_t)mcap))) return rc;
    if ((rc = S.take(head, (size_t)fcap + 1)) || (rc = S.take(rid, (size_t)fcap + 1)) || (rc = S.take(rstart, (size_t)capev + 1)) || (rc = S.take(ra, (size_t)capev)) ||
        (rc = S.take(rb, (size_t)capev)) || (rc = S.take(rc_, (size_t)capev)) || (rc = S.take(val, (size_t)fcap)) || (rc = S.take(keep, (size_t)fcap + 1)) ||
        (rc = S.take(kofs, (size_t)fcap + 1)) || (rc = S.take(carb, (size_t)nids + 1)) || (rc = S.take(carc, (size_t)nids + 1)) || (rc = S.take(mw, (size_t)mcap)) ||
        (rc = S.take(ma, (size_t)mcap)) || (rc = S.take(mb, (size_t)mcap)) || (rc = S.take(mc, (size_t)mcap)) || (rc = S.take(bnd, 2)))
        return rc;
    // (d) per chunk: sort the pairs by (A, B), count the runs; the runs of a pattern cut by the chunk's end are carried, merged with the next
    // chunk's runs of that pattern; every other run is final: valued, filtered, appended
    const int idbits = bits_for(nids);
    uint64_t  K = 0, kcap = 0;
    DevBuf<uint32_t> ca, cb, cc;
    DevBuf<double>   cv;
    auto finalize = [&](const uint32_t* fa, const uint32_t* fb, const uint32_t* fc, uint64_t n) -> int {  // final runs -> kept rows
        if (n == 0) return COLIBRI_OK;
        unsigned long long Kc = 0;
        int                r;
        hipLaunchKernelGGL(cooc_value_kernel, dim3(stream_grid(n)), dim3(kBlock), 0, c->stream, fa, fb, fc, n, cnt.p, npmi, threshold, npmi_threshold, (uint32_t)nrefs, val.p, keep.p);
        HIP_TRY(c, hipMemsetAsync(keep.p + n, 0, sizeof(uint32_t), c->stream));
        if ((r = scan_u32(c, keep.p, (uint32_t)n + 1, kofs.p, &Kc))) return r;
        if (K + Kc > kcap) {  // the kept rows so far: grow, keeping what they hold
            const uint64_t want = std::max<uint64_t>(K + Kc, kcap + kcap / 2) + 1;
            DevBuf<uint32_t> na, nb, nc;
            DevBuf<double>   nv;
            if ((r = S.take(na, (size_t)want)) || (r = S.take(nb, (size_t)want)) || (r = S.take(nc, (size_t)want)) || (r = S.take(nv, (size_t)want))) return r;
            if (K) {
                HIP_TRY(c, hipMemcpyAsync(na.p, ca.p, sizeof(uint32_t) * K, hipMemcpyDeviceToDevice, c->stream));
                HIP_TRY(c, hipMemcpyAsync(nb.p, cb.p, sizeof(uint32_t) * K, hipMemcpyDeviceToDevice, c->stream));
                HIP_TRY(c, hipMemcpyAsync(nc.p, cc.p, sizeof(uint32_t) * K, hipMemcpyDeviceToDevice, c->stream));
                HIP_TRY(c, hipMemcpyAsync(nv.p, cv.p, sizeof(double) * K, hipMemcpyDeviceToDevice, c->stream));
            }
            S.drop(ca); S.drop(cb); S.drop(cc); S.drop(cv);
            ca = std::move(na);
            cb = std::move(nb);
            cc = std::move(nc);
            cv = std::move(nv);
            kcap = want;
        }
        if (Kc) hipLaunchKernelGGL(cooc_compact_kernel, dim3(stream_grid(n)), dim3(kBlock), 0, c->stream, fa, fb, fc, val.p, keep.p, kofs.p, n, ca.p + K, cb.p + K, cc.p + K, cv.p + K);
        K += Kc;
        return COLIBRI_OK;
    };
    uint64_t ncarry = 0;  // runs of pattern hfirst[j] carried into chunk j (by B, ascending)
    for (uint32_t j = 0; j < nchunks; ++j) {
        const uint64_t k0 = hstart[j], k1 = hstart[j + 1], m = hbase[j + 1] - hbase[j];
        if (k0 == k1) continue;  // (an empty chunk: its boundary is the next one's)
        const uint32_t ahead = hfirst[j], atail = hlast[j + 1];
        const bool     open_start = hmid[j] != 0, open_end = hmid[j + 1] != 0;
        unsigned long long R = 0;
        if (m) {
            {
                Prof p(c, COLIBRI_K_EMIT);
                if (skc)
                    hipLaunchKernelGGL(skc_emit_kernel, dim3(stream_grid(k1 - k0)), dim3(kBlock), 0, c->stream, skc->cnum.p, aid.p, k0, k1, hbase[j], evoff.p, kb[0].p, ka[0].p);
                else if (rel < 0)
                    hipLaunchKernelGGL(cooc_emit_kernel, dim3(stream_grid((k1 - k0) * kCoocWave)), dim3(kBlock), 0, c->stream, k0, k1, hbase[j], nsent, c->first_sentence, evoff.p,
                                       V.rs, aid.p, V.rt, ntok.p, c->delimpos.p, ndelim, npos, boff.p, bpos.p, bn.p, bid.p, kb[0].p, ka[0].p);
                else if (rel == kRelSubchildren)
                    hipLaunchKernelGGL(rel_emit_kernel<kRelSubchildren>, dim3(stream_grid(k1 - k0)), dim3(kBlock), 0, c->stream, ra_, k0, k1, hbase[j], evoff.p, kb[0].p, ka[0].p);
                else if (rel == kRelSubparents)
                    hipLaunchKernelGGL(rel_emit_kernel<kRelSubparents>, dim3(stream_grid(k1 - k0)), dim3(kBlock), 0, c->stream, ra_, k0, k1, hbase[j], evoff.p, kb[0].p, ka[0].p);
                else if (rel == kRelLeft)
                    hipLaunchKernelGGL(rel_emit_kernel<kRelLeft>, dim3(stream_grid(k1 - k0)), dim3(kBlock), 0, c->stream, ra_, k0, k1, hbase[j], evoff.p, kb[0].p, ka[0].p);
                else if (rel == kRelInstances)
                    hipLaunchKernelGGL(rel_emit_kernel<kRelInstances>, dim3(stream_grid(k1 - k0)), dim3(kBlock), 0, c->stream, ra_, k0, k1, hbase[j], evoff.p, kb[0].p, ka[0].p);
                else if (rel == kRelTemplates)
                    hipLaunchKernelGGL(rel_emit_kernel<kRelTemplates>, dim3(stream_grid(k1 - k0)), dim3(kBlock), 0, c->stream, ra_, k0, k1, hbase[j], evoff.p, kb[0].p, ka[0].p);
                else
                    hipLaunchKernelGGL(rel_emit_kernel<kRelRight>, dim3(stream_grid(k1 - k0)), dim3(kBlock), 0, c->stream, ra_, k0, k1, hbase[j], evoff.p, kb[0].p, ka[0].p);
            }
            int c2 = 0;
            {
                Prof p(c, COLIBRI_K_SCATTER);
                uint32_t* const bk[2] = {kb[0].p, kb[1].p};
                uint32_t* const ak[2] = {ka[0].p, ka[1].p};
                if ((rc = radix_sort_pairs(c, bk, ak, m, idbits, c2)) || (rc = radix_sort_pairs(c, ak, bk, m, idbits, c2))) return rc;  // by B, then (stable) by A
            }
            hipLaunchKernelGGL(cooc_heads_kernel, dim3(stream_grid(m)), dim3(kBlock), 0, c->stream, ka[c2].p, kb[c2].p, m, head.p);
            HIP_TRY(c, hipMemsetAsync(head.p + m, 0, sizeof(uint32_t), c->stream));
            if ((rc = scan_u32(c, head.p, (uint32_t)m + 1, rid.p, &R))) return rc;
            hipLaunchKernelGGL(cooc_runs_kernel, dim3(stream_grid(m)), dim3(kBlock), 0, c->stream, ka[c2].p, kb[c2].p, head.p, rid.p, m, ra.p, rb.p, rstart.p);
            hipLaunchKernelGGL(cooc_runlen_kernel, dim3(stream_grid(R)), dim3(kBlock), 0, c->stream, rstart.p, (uint64_t)R, m, rc_.p);
        }
        // runs [0, h) are pattern ahead's, [t, R) pattern atail's (the runs are sorted by A, and A only grows along the references)
        unsigned long long hb[2] = {0, 0};
        if (R) {
            hipLaunchKernelGGL(cooc_bounds_kernel, dim3(1), dim3(1), 0, c->stream, ra.p, (uint64_t)R, ahead, atail, bnd.p);
            HIP_TRY(c, hipMemcpyAsync(hb, bnd.p, sizeof hb, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
        }
        const uint64_t h = hb[0], t = hb[1];
        // pattern ahead's runs: merged with the carried ones when the chunk starts inside that pattern
        const uint32_t *ha = ra.p, *hbp = rb.p, *hc = rc_.p;
        uint64_t        hn = h;
        if (open_start) {
            const uint64_t n2 = ncarry + h;
            unsigned long long M = 0;
            if (n2) {
                if (ncarry) {
                    HIP_TRY(c, hipMemcpyAsync(mk[0].p, carb.p, sizeof(uint32_t) * ncarry, hipMemcpyDeviceToDevice, c->stream));
                    HIP_TRY(c, hipMemcpyAsync(mw.p, carc.p, sizeof(uint32_t) * ncarry, hipMemcpyDeviceToDevice, c->stream));
                }
                if (h) {
                    HIP_TRY(c, hipMemcpyAsync(mk[0].p + ncarry, rb.p, sizeof(uint32_t) * h, hipMemcpyDeviceToDevice, c->stream));
                    HIP_TRY(c, hipMemcpyAsync(mw.p + ncarry, rc_.p, sizeof(uint32_t) * h, hipMemcpyDeviceToDevice, c->stream));
                }
                int             c3    = 0;
                uint32_t* const kk[2] = {mk[0].p, mk[1].p};
                uint32_t* const pp[2] = {mp[0].p, mp[1].p};
                hipLaunchKernelGGL(cooc_iota_kernel, dim3(stream_grid(n2)), dim3(kBlock), 0, c->stream, mp[0].p, n2);
                if ((rc = radix_sort_pairs(c, kk, pp, n2, idbits, c3))) return rc;
                hipLaunchKernelGGL(cooc_heads_kernel, dim3(stream_grid(n2)), dim3(kBlock), 0, c->stream, mk[c3].p, mk[c3].p, n2, head.p);
                HIP_TRY(c, hipMemsetAsync(head.p + n2, 0, sizeof(uint32_t), c->stream));
                if ((rc = scan_u32(c, head.p, (uint32_t)n2 + 1, rid.p, &M))) return rc;
                HIP_TRY(c, hipMemsetAsync(mc.p, 0, sizeof(uint32_t) * M, c->stream));
                hipLaunchKernelGGL(cooc_mergeb_kernel, dim3(stream_grid(n2)), dim3(kBlock), 0, c->stream, mk[c3].p, head.p, rid.p, n2, mw.p, mp[c3].p, ahead, ma.p, mb.p, mc.p);
            }
            ha = ma.p, hbp = mb.p, hc = mc.p, hn = M;
        }
        ncarry = 0;
        if (open_end && atail == ahead) {  // the chunk lies inside one pattern: all of it is carried on
            if (hn) {
                HIP_TRY(c, hipMemcpyAsync(carb.p, hbp, sizeof(uint32_t) * hn, hipMemcpyDeviceToDevice, c->stream));
                HIP_TRY(c, hipMemcpyAsync(carc.p, hc, sizeof(uint32_t) * hn, hipMemcpyDeviceToDevice, c->stream));
            }
            ncarry = hn;
            continue;
        }
        if ((rc = finalize(ha, hbp, hc, hn))) return rc;
        const uint64_t close_end = open_end ? t : R;  // runs [h, close_end) are final; [t, R) are carried when the chunk ends inside pattern atail
        if (close_end > h && (rc = finalize(ra.p + h, rb.p + h, rc_.p + h, close_end - h))) return rc;
        if (open_end && R > t) {
            HIP_TRY(c, hipMemcpyAsync(carb.p, rb.p + t, sizeof(uint32_t) * (R - t), hipMemcpyDeviceToDevice, c->stream));
            HIP_TRY(c, hipMemcpyAsync(carc.p, rc_.p + t, sizeof(uint32_t) * (R - t), hipMemcpyDeviceToDevice, c->stream));
            ncarry = R - t;
        }
    }
    if (K >= 0xFFFFFFF0ull) return fail(c, COLIBRI_ERR_OVERFLOW, "%s: %llu rows", what, (unsigned long long)K);
    for (int i = 0; i < 2; ++i) { S.drop(ka[i]); S.drop(kb[i]); S.drop(mk[i]); S.drop(mp[i]); }
    S.drop(head); S.drop(rid); S.drop(rstart); S.drop(ra); S.drop(rb); S.drop(rc_); S.drop(val); S.drop(keep); S.drop(kofs);
    S.drop(carb); S.drop(carc); S.drop(mw); S.drop(ma); S.drop(mb); S.drop(mc); S.drop(bnd);
    // the order: value descending, then A's key bytes, then B's key bytes (ranks of the patterns by key bytes: LSD over four-byte groups);
    // relations: A's pattern number, then count descending, then B's key bytes
    if ((rc = dev_alloc(c, co.a, (size_t)K + 1)) || (rc = dev_alloc(c, co.b, (size_t)K + 1)) || (rc = dev_alloc(c, co.cnt, (size_t)K + 1)) || (rc = dev_alloc(c, co.val, (size_t)K + 1)))
        return rc;
    if (K) {
        // (the skip content ranks its own B side: the distinct contents' bytes)
        const uint8_t*            bkeys = skc ? skc->dbytes.p : V.kbytes;
        const unsigned long long* bkoff = skc ? skc->doff.p : V.koff;
        const uint32_t            nb = skc ? (uint32_t)skc->nd : np, bmax = skc ? skc->maxlen : maxkey;
        const uint64_t big = std::max<uint64_t>(nb, K) + 1;
        for (int i = 0; i < 2; ++i)
            if ((rc = S.take(perm[i], (size_t)big)) || (rc = S.take(key[i], (size_t)big))) return rc;
        if ((rc = S.take(rank, (size_t)nb + 1))) return rc;
        uint32_t* const kk[2] = {key[0].p, key[1].p};
        uint32_t* const pp[2] = {perm[0].p, perm[1].p};
        int             c4    = 0;
        hipLaunchKernelGGL(cooc_iota_kernel, dim3(stream_grid(nb)), dim3(kBlock), 0, c->stream, perm[0].p, (uint64_t)nb);
        hipLaunchKernelGGL(cooc_keychunk_kernel, dim3(stream_grid(nb)), dim3(kBlock), 0, c->stream, bkeys, bkoff, perm[0].p, nb, kInvalid, key[0].p);
        if ((rc = radix_sort_pairs(c, kk, pp, nb, bits_for((uint64_t)bmax + 1), c4))) return rc;
        for (int ch = (int)((bmax + 3) / 4) - 1; ch >= 0; --ch) {
            hipLaunchKernelGGL(cooc_keychunk_kernel, dim3(stream_grid(nb)), dim3(kBlock), 0, c->stream, bkeys, bkoff, perm[c4].p, nb, (uint32_t)ch, key[c4].p);
            if ((rc = radix_sort_pairs(c, kk, pp, nb, 32, c4))) return rc;
        }
        hipLaunchKernelGGL(cooc_rank_kernel, dim3(stream_grid(nb)), dim3(kBlock), 0, c->stream, perm[c4].p, nb, rank.p);
        c4 = 0;
        hipLaunchKernelGGL(cooc_iota_kernel, dim3(stream_grid(K)), dim3(kBlock), 0, c->stream, perm[0].p, (uint64_t)K);
        hipLaunchKernelGGL(cooc_gather2_kernel, dim3(stream_grid(K)), dim3(kBlock), 0, c->stream, rank.p, cb.p, perm[0].p, (uint64_t)K, key[0].p);
        if ((rc = radix_sort_pairs(c, kk, pp, K, idbits, c4))) return rc;  // (a rank is below the B side's size: idbits hold it)
        if (rel < 0) {
            hipLaunchKernelGGL(cooc_gather2_kernel, dim3(stream_grid(K)), dim3(kBlock), 0, c->stream, rank.p, ca.p, perm[c4].p, (uint64_t)K, key[c4].p);
            if ((rc = radix_sort_pairs(c, kk, pp, K, idbits, c4))) return rc;
            for (int half = 0; half < 2; ++half) {
                hipLaunchKernelGGL(cooc_valkey_kernel, dim3(stream_grid(K)), dim3(kBlock), 0, c->stream, cv.p, perm[c4].p, (uint64_t)K, half, key[c4].p);
                if ((rc = radix_sort_pairs(c, kk, pp, K, 32, c4))) return rc;
            }
        } else {
            hipLaunchKernelGGL(rel_countkey_kernel, dim3(stream_grid(K)), dim3(kBlock), 0, c->stream, cc.p, perm[c4].p, (uint64_t)K, key[c4].p);
            if ((rc = radix_sort_pairs(c, kk, pp, K, 32, c4))) return rc;
            hipLaunchKernelGGL(cooc_gather_kernel, dim3(stream_grid(K)), dim3(kBlock), 0, c->stream, ca.p, perm[c4].p, (uint64_t)K, key[c4].p);
            if ((rc = radix_sort_pairs(c, kk, pp, K, bits_for(np), c4))) return rc;
        }
        hipLaunchKernelGGL(cooc_permute_kernel, dim3(stream_grid(K)), dim3(kBlock), 0, c->stream, perm[c4].p, (uint64_t)K, ca.p, cb.p, cc.p, cv.p, co.a.p, co.b.p, co.cnt.p, co.val.p);
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    collect_events(c);
    co.nrows   = K;
    co.events  = E;
    co.chunks  = nchunks;
    co.scratch = S.peak;
    co.valid   = true;
    *nrows     = K;
    return COLIBRI_OK;
}

static int cooc_begin(colibri_ctx* c, int mode, uint64_t* nrows) {
    if (!c || !nrows || (mode != COLIBRI_COOC_COUNT && mode != COLIBRI_COOC_NPMI)) return COLIBRI_ERR_ARG;
    auto& co = c->co;
    co.valid = false;
    co.nrows = co.events = co.scratch = 0;
    co.chunks = 0;
    *nrows    = 0;
    if (!c->have_corpus) return fail(c, COLIBRI_ERR_STATE, "cooc needs the corpus uploaded (colibri_upload_corpus): it is the reverse index");
    return COLIBRI_OK;
}

int colibri_cooc(colibri_ctx* c, const uint64_t* key_off, const uint8_t* key_bytes, const uint64_t* ref_off, const uint32_t* ref_sentence, const uint16_t* ref_token, uint64_t npatterns,
                 uint32_t threshold, int mode, double npmi_threshold, uint64_t* nrows) {
    int rc = cooc_begin(c, mode, nrows);
    if (rc) return rc;
    if (npatterns == 0) {
        c->co.valid = true;
        return COLIBRI_OK;
    }
    ModelView V;
    if ((rc = model_upload(c, "cooc", key_off, key_bytes, nullptr, ref_off, ref_sentence, ref_token, npatterns, kModelIndexed, V))) return rc;
    return cooc_core(c, V, threshold, mode == COLIBRI_COOC_NPMI, npmi_threshold, nrows);
}

// the same on the indexed model of the last colibri_train of this context, still resident in HBM with its corpus
int colibri_cooc_resident(colibri_ctx* c, uint32_t threshold, int mode, double npmi_threshold, uint64_t* nrows) {
    int rc = cooc_begin(c, mode, nrows);
    if (rc) return rc;
    ModelView V;
    if ((rc = model_resident(c, "colibri_cooc_resident", true, V))) return rc;
    if (V.np == 0) {
        c->co.valid = true;
        return COLIBRI_OK;
    }
    return cooc_core(c, V, threshold, mode == COLIBRI_COOC_NPMI, npmi_threshold, nrows);
}

int colibri_cooc_fetch(colibri_ctx* c, uint32_t* pattern_a, uint32_t* pattern_b, uint32_t* counts, double* values) {
    if (!c) return COLIBRI_ERR_ARG;
    auto& co = c->co;
    if (!co.valid) return fail(c, COLIBRI_ERR_STATE, "colibri_cooc / colibri_cooc_resident first");
    const uint64_t K = co.nrows;
    if (!K) return COLIBRI_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    if (pattern_a) HIP_TRY(c, hipMemcpyAsync(pattern_a, co.a.p, sizeof(uint32_t) * K, hipMemcpyDeviceToHost, c->stream));
    if (pattern_b) HIP_TRY(c, hipMemcpyAsync(pattern_b, co.b.p, sizeof(uint32_t) * K, hipMemcpyDeviceToHost, c->stream));
    if (counts) HIP_TRY(c, hipMemcpyAsync(counts, co.cnt.p, sizeof(uint32_t) * K, hipMemcpyDeviceToHost, c->stream));
    if (values) HIP_TRY(c, hipMemcpyAsync(values, co.val.p, sizeof(double) * K, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return COLIBRI_OK;
}

int colibri_cooc_info(const colibri_ctx* c, uint64_t* events, uint64_t* chunks, uint64_t* scratch_bytes) {
    if (!c) return COLIBRI_ERR_ARG;
    if (events) *events = c->co.events;
    if (chunks) *chunks = c->co.chunks;
    if (scratch_bytes) *scratch_bytes = c->co.scratch;
    return COLIBRI_OK;
}
