// kshard_api.inc — part of colibri_hip.hip (same translation unit, inside its extern "C" block): the colibri_kshard_* entry points of the C ABI —
// key-sharded counting (kshard2.hpp; the routes and order 1 from kshard.hpp), the multi-GPU form of the plain n-gram run. The collectives are the caller's (host/src/sharded.cpp: RCCL linked directly, or
// device copies between contexts that share a device); everything here is enqueued on the context's own stream (colibri_stream), which the caller also hands to
// RCCL, so an order costs two host look-ups (the sizes of the two exchanges) and nothing else waits.
//   per run    colibri_kshard_info (every rank; the caller checks that all agree) -> colibri_kshard_begin
//   order 1    colibri_kshard_uni_count -> [all-reduce SUM of the dense class counts] -> colibri_kshard_uni_apply
//   order n>1  colibri_kshard_emit -> [all-to-all: 4-byte keys + per-(owner, bin) tables; order 2: all-reduce of the dense head] -> colibri_kshard_count ->
//              [all-to-all: feedback (a bit per key + a number per surviving key) + exports; all-gather of the owners' kept counts] -> colibri_kshard_apply
//   end        colibri_kshard_local_stats -> [sum over ranks] -> colibri_kshard_finish, then the usual colibri_result_sizes / colibri_export_unindexed per rank:
//              every pattern of the model is exported by exactly one rank (the lowest one holding an occurrence of it).

}  // extern "C" (the helpers below are C++)

namespace {

constexpr uint32_t kKsRouteLen = 32768;  // entries per list of a flat route
constexpr uint32_t kKsFlatCap  = 16384;  // piece length when bi2_pospart_kernel walks the received positions

uint32_t ks_range_shift(uint64_t maxclass) {
    uint32_t shift = 12;
    while (shift <= 14 && (maxclass >> shift) >= (uint64_t)kUniBins) ++shift;
    return shift > 14 ? 0u : shift;
}
inline uint32_t ks_log2(int world) {
    uint32_t w = 0;
    while ((1 << w) < world) ++w;
    return w;
}
TrainPlan ks_plan(const colibri_ctx* c) {
    TrainPlan pl{};
    pl.npos     = c->npos;
    pl.thr      = (uint32_t)c->opt.mintokens;
    pl.res_cap  = 0;
    constexpr uint32_t kCountLdsBytes    = kCountTile * 16u + kCountLSlot * 4u + 64u;
    constexpr uint32_t kCountBlocksPerCU = (160u * 1024u / kCountLdsBytes) < 8u ? (160u * 1024u / kCountLdsBytes) : 8u;
    pl.cnt_grid = std::max<uint32_t>(1, std::min<uint32_t>(blocks_for(c->npos, kCountTile), 256u * kCountBlocksPerCU));
    pl.pos_grid = stream_grid(c->npos);
    return pl;
}
template <class T>
int ks_bytes(colibri_ctx* c, DevBuf<T>& b, uint64_t n) {
    if (b.p && b.n >= n) return COLIBRI_OK;
    return dev_alloc(c, b, (size_t)(n + n / 8 + 256));
}

// the three kernels of a route: per-list counts, their places, the move. `slot` (0 / 1): which half of the count / place arrays (two routes of a pass are
// counted and placed before either moves, so that the host can look at both totals while the moves run)
template <class Spec>
void ks_route_count(colibri_ctx* c, const Spec& sp, uint32_t nlists, uint32_t world, KsRouteState* rs, int slot) {
    auto&           ks   = c->ks;
    uint32_t* const lcnt = ks.lcnt.p + (size_t)slot * (ks.lcnt.n / 2), *loff = ks.loff.p + (size_t)slot * (ks.loff.n / 2);
    if (nlists) hipLaunchKernelGGL((ks_route_hist_kernel<Spec>), dim3(std::min<uint32_t>(nlists, 2048u)), dim3(kKsThreads), 0, c->stream, sp, nlists, lcnt);
    hipLaunchKernelGGL(ks_route_scan_kernel, dim3(1), dim3(kKsThreads), 0, c->stream, (const uint32_t*)lcnt, loff, nlists, world, rs);
}
template <class Spec, int PER>
void ks_route_move(colibri_ctx* c, const Spec& sp, uint32_t nlists, uint32_t world, typename Spec::Out* out, int slot) {
    auto&                 ks   = c->ks;
    const uint32_t* const loff = ks.loff.p + (size_t)slot * (ks.loff.n / 2);
    if (nlists) hipLaunchKernelGGL((ks_route_move_kernel<Spec, PER>), dim3(std::min<uint32_t>(nlists, 2048u)), dim3(kKsThreads), 0, c->stream, sp, nlists, loff, world, out);
}

// The host's look at a few words the stream has JUST produced, while the kernels enqueued after them run: an event on the main stream, a side stream that waits
// for it and copies into pinned memory. ks_peek_begin: mark the point; ks_peek: enqueue one copy (words at `word_off` of the pinned block); ks_peek_end: wait.
int ks_peek_begin(colibri_ctx* c) {
    auto& ks = c->ks;
    if (!ks.side) {
        HIP_TRY(c, hipStreamCreateWithFlags(&ks.side, hipStreamNonBlocking));
        HIP_TRY(c, hipEventCreateWithFlags(&ks.ev, hipEventDisableTiming));
        HIP_TRY(c, hipHostMalloc((void**)&ks.pinned, sizeof(uint32_t) * 128, hipHostMallocDefault));
    }
    HIP_TRY(c, hipEventRecord(ks.ev, c->stream));
    HIP_TRY(c, hipStreamWaitEvent(ks.side, ks.ev, 0));
    return COLIBRI_OK;
}
int ks_peek(colibri_ctx* c, uint32_t word_off, const void* src, size_t bytes) {
    HIP_TRY(c, hipMemcpyAsync(c->ks.pinned + word_off, src, bytes, hipMemcpyDeviceToHost, c->ks.side));
    return COLIBRI_OK;
}
int ks_peek_end(colibri_ctx* c) {
    HIP_TRY(c, hipStreamSynchronize(c->ks.side));
    HIP_TRY(c, hipGetLastError());
    ++c->ks.syncs;
    return COLIBRI_OK;
}

}  // namespace

extern "C" {

void* colibri_stream(colibri_ctx* c) { return c ? (void*)c->stream : nullptr; }

// tokens per rank the protocol takes: an owner's final bins hold (tokens per rank) / 131 072 records of order 2 — the single-device engine's bins, whose 1024-slot
// tables carry one pass of 2.15 x 10^8 positions (colibri_hip.hip kNarrowPassPositions). Round 4 stopped at 1.28 x 10^8 (a rank of the 8 x 125 M run sat 2.4 % under
// it); a run whose bins do overflow is repeated on the candidate exchange, as before.
constexpr uint64_t kKsMaxTokens = 200ull * 1000 * 1000;
int colibri_kshard_info(colibri_ctx* c, const colibri_options* opt_in, int* eligible, uint64_t* maxclass, uint64_t* npositions) {
    if (!c || !opt_in || !eligible || !maxclass || !npositions) return COLIBRI_ERR_ARG;
    if (!c->have_corpus) return fail(c, COLIBRI_ERR_STATE, "no corpus uploaded");
    colibri_options o = *opt_in;
    const int       rc = check_options(c, o);
    *maxclass    = c->maxclass;
    *npositions  = c->npos;
    *eligible    = rc == COLIBRI_OK && c->cs.n == 0 && !o.doskipgrams && !o.doskipgrams_exhaustive && !o.dopatternperline && o.maxbackofflength >= o.maxlength &&
                o.table_mode == 0 && !(c->flags & kFlagNonCanonical) && c->maxclass < (1u << 21) && c->ntokens <= kKsMaxTokens && c->npos < (1u << 28) &&
                !getenv("COLIBRI_NO_KSHARD");
    return COLIBRI_OK;
}

int colibri_kshard_begin(colibri_ctx* c, const colibri_options* opt_in, int world, int rank, uint64_t maxclass_global, uint64_t maxpos_global) {
    if (!c || !opt_in || world < 1 || world > kKsWorld || (world & (world - 1)) || rank < 0 || rank >= world) return COLIBRI_ERR_ARG;
    if (!c->have_corpus) return fail(c, COLIBRI_ERR_STATE, "no corpus uploaded");
    c->b2.keep.drop();  // (the sharded trainers write order 2's state and lists their own way: nothing kept outlives them)
    colibri_options o = *opt_in;
    int             rc;
    if ((rc = check_options(c, o))) return rc;
    if (maxclass_global < c->maxclass || maxclass_global >= (1u << 21) || maxpos_global < c->npos || maxpos_global >= (1u << 28))
        return fail(c, COLIBRI_ERR_UNSUPPORTED, "key-sharded counting needs class ids below 2^21 and fewer than 2^28 positions per rank");
    HIP_TRY(c, hipSetDevice(c->device));
    auto& ks   = c->ks;
    c->opt     = o;
    c->trained = false;
    c->profile = o.profile;
    collect_events(c);
    std::fill(std::begin(c->k_ms), std::end(c->k_ms), 0.0);
    std::fill(std::begin(c->k_launches), std::end(c->k_launches), 0);
    c->profile_class = COLIBRI_K_COUNT2;
    c->segments.clear();
    c->npairs = 0;
    c->sh.active = false;
    c->ks.ran    = false;
    const uint32_t npos = c->npos;
    ks.world     = world;
    ks.rank      = rank;
    ks.w         = ks_log2(world);
    ks.nclasses  = (uint32_t)maxclass_global + 1;
    ks.uni_shift = ks_range_shift(maxclass_global);
    if (!ks.uni_shift) return fail(c, COLIBRI_ERR_UNSUPPORTED, "key-sharded counting: class space too large for the partitioned order 1");
    ks.clsbits = 1;
    while ((1ull << ks.clsbits) <= maxclass_global) ++ks.clsbits;
    ks.posbits = 1;
    while ((1ull << ks.posbits) < maxpos_global + 1) ++ks.posbits;
    ks.posbits = std::max(ks.posbits, 20u);
    const uint32_t K = std::max(2u * ks.clsbits, 17u + ks.w);
    if (K - 8 + ks.posbits > 64 || K > 48u + ks.w) return fail(c, COLIBRI_ERR_UNSUPPORTED, "key-sharded counting: key and position do not fit a record");
    ks.kbits = K;
    // source side: what the single-device run of this corpus has
    if ((rc = dev_alloc(c, c->cnt1, (size_t)ks.nclasses + 2)) || (rc = dev_alloc(c, c->unistate, 1)) || (rc = dev_alloc(c, c->uni_tail, uni_tail_words(npos))) ||
        (rc = dev_alloc(c, c->uni_rows, (size_t)kUniHeadGrid * kUniHead)) || (rc = dev_alloc(c, c->uni_surv, (size_t)ks.nclasses / 32 + 4 + kBi2SurvLds)))
        return rc;
    if (c->ids.size() < 2) c->ids.resize(2);
    if ((rc = dev_alloc(c, c->ids[0], (size_t)npos + 1)) || (rc = dev_alloc(c, c->ids[1], (size_t)npos + 1))) return rc;
    if ((rc = dev_alloc(c, c->recs[0], ((size_t)npos + (npos >> 2)) / kBins * kBins + (size_t)kBins * kScatTile * 4)) ||
        (rc = dev_alloc(c, c->recs[1], std::max<size_t>((size_t)npos + 1, (size_t)kBins * kScatTile * 4))))
        return rc;
    if ((rc = dev_alloc(c, c->rep_of, (size_t)npos + 1)) || (rc = dev_alloc(c, c->ids_at, (size_t)npos + 1)) || (rc = dev_alloc(c, c->binstate, 1))) return rc;
    if ((rc = dev_alloc(c, c->alist[0], (size_t)npos + 1)) || (rc = dev_alloc(c, c->alist[1], (size_t)npos + 1)) || (rc = dev_alloc(c, c->alist_n, 2))) return rc;
    if ((rc = bigram2_alloc(c, npos, /*chain=*/true))) return rc;
    if ((rc = dev_alloc(c, c->state, 1))) return rc;
    // exchange and owner side: the small fixed pieces (the large ones follow the sizes of each pass)
    if ((rc = dev_alloc(c, ks.split, 1)) || (rc = dev_alloc(c, ks.rstate, 2)) || (rc = dev_alloc(c, ks.stats, 1)) || (rc = dev_alloc(c, ks.ostate, 1)) ||
        (rc = dev_alloc(c, ks.obs, 1)) || (rc = dev_alloc(c, ks.obin, 1)) || (rc = dev_alloc(c, ks.slotbase, kKsSlots)) || (rc = dev_alloc(c, ks.tab_recv, (size_t)kKsWorld * kKs2Bins)) ||
        (rc = dev_alloc(c, ks.headg, 2 * (size_t)kBi2HeadN)) || (rc = dev_alloc(c, ks.oboff, (size_t)kKsSlots * (kBi2BBins + 1))) || (rc = dev_alloc(c, ks.ks2, 1)) ||
        (rc = dev_alloc(c, ks.fbinfo, 1)) || (rc = dev_alloc(c, ks.tab, (size_t)kKsWorld * kKs2Bins)) || (rc = dev_alloc(c, ks.key4, (size_t)npos + 64)) ||
        (rc = dev_alloc(c, ks.posbuf, (size_t)npos + 64)) || (rc = dev_alloc(c, ks.rowtot, kKsSlots)) || (rc = dev_alloc(c, ks.zero8k, 2 * (size_t)kBi2HeadN)) ||
        (rc = dev_alloc(c, ks.small, 16)) || (rc = dev_alloc(c, ks.cbhist, (size_t)kKsSlots * 8 * kBi2BBins)))
        return rc;
    HIP_TRY(c, hipMemsetAsync(ks.zero8k.p, 0, sizeof(uint32_t) * 2 * kBi2HeadN, c->stream));
    ks.indexed = o.indexed != 0;
    ks.gid_off = 0;
    if (ks.indexed && ((rc = pairs_begin(c, npos)) || (rc = dev_alloc(c, ks.fin_gid, (size_t)ks.nclasses + (size_t)npos / 4 + 1024)))) return rc;
    if ((rc = dev_alloc(c, ks.fin_rep, (size_t)ks.nclasses + (size_t)npos / 4 + 1024)) || (rc = dev_alloc(c, ks.fin_cnt, ks.fin_rep.n))) return rc;
    HIP_TRY(c, hipMemsetAsync(ks.stats.p, 0, sizeof(KsStats), c->stream));
    HIP_TRY(c, hipMemsetAsync(ks.ostate.p, 0, sizeof(DevState), c->stream));
    HIP_TRY(c, hipMemsetAsync(c->state.p, 0, sizeof(DevState), c->stream));
    std::memset(&c->hstate, 0, sizeof c->hstate);
    std::memset(&c->stats, 0, sizeof c->stats);
    ks.fin_total   = 0;
    ks.n           = 0;
    ks.pending_uni = false;
    ks.syncs       = 0;
    ks.active      = true;
    return COLIBRI_OK;
}

// order 1: this rank's dense class counts (kernels.hpp section 2b: LDS head histogram + partitioned tail, no per-token global atomic). The caller all-reduces
// cnt_dev[0 .. nclasses) (SUM, u32) in place — the north star's "all-reduce of the per-bucket count tables before the prune" — on colibri_stream.
int colibri_kshard_uni_count(colibri_ctx* c, void** cnt_dev, uint32_t* nclasses) {
    if (!c || !cnt_dev || !nclasses) return COLIBRI_ERR_ARG;
    if (!c->ks.active) return fail(c, COLIBRI_ERR_STATE, "colibri_kshard_begin first");
    HIP_TRY(c, hipSetDevice(c->device));
    int rc;
    if ((rc = uni_count_partitioned(c, c->ks.uni_shift, c->cnt1.p, c->ks.nclasses))) return rc;
    *cnt_dev  = c->cnt1.p;
    *nclasses = c->ks.nclasses;
    c->ks.n   = 1;
    return COLIBRI_OK;
}
// ... and the threshold on the reduced array: the same survivors on every rank (bitmap for order 2's look-back); rank 0 exports the unigrams (from their class ids)
int colibri_kshard_uni_apply(colibri_ctx* c) {
    if (!c) return COLIBRI_ERR_ARG;
    auto& ks = c->ks;
    if (!ks.active || ks.n != 1) return fail(c, COLIBRI_ERR_STATE, "colibri_kshard_uni_apply out of order");
    HIP_TRY(c, hipSetDevice(c->device));
    int rc;
    if ((rc = ks_bytes(c, ks.ores_rep, (uint64_t)ks.nclasses + 64)) || (rc = ks_bytes(c, ks.ores_cnt, (uint64_t)ks.nclasses + 64))) return rc;
    const uint32_t wthr = c->opt.mintokens_unigrams > c->opt.mintokens ? (uint32_t)c->opt.mintokens_unigrams : 0u;
    {
        Prof p(c, COLIBRI_K_PRUNE);
        // (rank 0 writes the results straight into its share of the model; the others only need the figures and the bitmap)
        uint32_t* const rep = ks.rank == 0 ? ks.fin_rep.p : ks.ores_rep.p;
        uint32_t* const cnt = ks.rank == 0 ? ks.fin_cnt.p : ks.ores_cnt.p;
        hipLaunchKernelGGL(uni_finish_kernel, dim3(stream_grid(ks.nclasses)), dim3(kBlock), 0, c->stream, (const uint32_t*)c->cnt1.p, (const uint32_t*)nullptr, ks.nclasses,
                           (uint32_t)c->opt.mintokens, ks.ostate.p, rep, cnt, (uint32_t)std::min<size_t>(ks.rank == 0 ? ks.fin_rep.n : ks.ores_rep.n, 0x7FFFFFF0u),
                           reinterpret_cast<uint16_t*>(c->uni_surv.p), false, (uint32_t*)nullptr, wthr);
        if (ks.indexed && ks.rank == 0)  // (the unigrams' numbers are their class ids)
            hipLaunchKernelGGL(ks2_export_gids_kernel, dim3(stream_grid(ks.nclasses)), dim3(kBlock), 0, c->stream, (const uint32_t*)ks.fin_rep.p,
                               (uint32_t)std::min<size_t>(ks.nclasses, ks.fin_gid.n), (const uint32_t*)nullptr, true, ks.fin_gid.p);
        hipLaunchKernelGGL(ks_order_end_kernel, dim3(1), dim3(1), 0, c->stream, ks.ostate.p, c->state.p, ks.stats.p, 1, 0xFFFFFFFFu);
    }
    if (ks.indexed) {  // the local references of every surviving word (threshold MINTOKENS: the word threshold only gates longer windows)
        const TrainPlan pl = ks_plan(c);
        int             rc2;
        hipLaunchKernelGGL(ks2_uni_ids_kernel, dim3(pl.pos_grid), dim3(kBlock), 0, c->stream, (const uint32_t*)c->cls.p, (const uint32_t*)c->cnt1.p, (uint32_t)c->opt.mintokens, c->npos,
                           c->ids[0].p);
        c->hstate.done = 0;
        if ((rc2 = emit_pairs(c, pl, c->ids[0].p, true))) return rc2;
        ++ks.syncs;
        ks.gid_off = ks.nclasses;
    }
    ks.pending_uni = true;  // the number of unigrams kept reaches the host with the next look-up
    return COLIBRI_OK;
}

}  // extern "C"
namespace {
// host figures of order 1, fetched with the first look-up that follows it
int ks_settle_uni(colibri_ctx* c) {
    auto& ks = c->ks;
    if (!ks.pending_uni) return COLIBRI_OK;
    uint32_t kept = 0;
    HIP_TRY(c, hipMemcpyAsync(&kept, &ks.stats.p->kept[1], sizeof kept, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    ks.pending_uni = false;
    if (ks.rank == 0) {
        if (kept) c->segments.push_back({0u, kept, 1, kMaskFromClass});
        ks.fin_total = kept;
    }
    return COLIBRI_OK;
}
}  // namespace
extern "C" {

// bshift every rank uses for an order with at most `est` records in all (so ~est / world per owner): <= ~700 records per final bin, at least 8 B bins, and the 31-bit
// in-bin key must hold every mix bit the bin does not fix (K - 17 - w + bshift <= 31)
static uint32_t ks2_bshift(uint64_t est, int world, uint32_t K, uint32_t w) {
    const uint64_t tot = est / (uint64_t)world + 1;
    uint32_t       nb  = 8;
    while (nb < (uint32_t)kBi2BBins && (uint64_t)nb * kBins * 700u < tot) nb <<= 1;
    uint32_t sh = 0;
    while ((uint32_t)kBi2BBins >> sh > nb) ++sh;
    const uint32_t maxsh = K >= 48u + w ? 0u : 48u + w - K;
    return std::min(sh, maxsh);
}

// order n >= 2, source side: scan -> records by A bin (the single-device emit kernels) -> level B -> (owner, A', B) runs of 4-byte in-bin keys. est_records: an upper
// bound of the order's records over ALL ranks (order 2: the corpus' tokens; above: the windows that survived the order below), ids_global: the numbers the order below
// handed out over all ranks (orders >= 3: they size the key) — the same values on every rank. On return (one look-up):
//   *send_dev      the keys, grouped by owner (per_owner[d] of them for rank d, in rank order), 4 bytes each
//   *tab_dev       u32[world][*tab_words]: records per (owner, A', B) — row d travels to rank d with its keys
//   *head_dev      order 2 only, else NULL: u32[2][4096], the dense head — the caller all-reduces row 0 (SUM) and row 1 (MIN) in place before colibri_kshard_count
//   *admitted      windows this rank counted at this order (the order loop ends when no rank counts any: "None found", patternmodel.h:1189-1194)
int colibri_kshard_emit(colibri_ctx* c, int n, uint64_t est_records, uint64_t ids_global, int more, void** send_dev, void** tab_dev, uint32_t* tab_words, uint64_t* per_owner,
                        uint32_t* recbytes, void** head_dev, uint64_t* admitted) {
    if (!c || !send_dev || !tab_dev || !tab_words || !per_owner || !recbytes || !head_dev || !admitted || n < 2 || n >= COLIBRI_MAX_ORDER) return COLIBRI_ERR_ARG;
    auto& ks = c->ks;
    if (!ks.active || n != ks.n + 1) return fail(c, COLIBRI_ERR_STATE, "colibri_kshard_emit out of order");
    HIP_TRY(c, hipSetDevice(c->device));
    const uint32_t    npos = c->npos;
    const Bigram2Plan b    = bigram2_plan(c, npos, kBi2SubWide);
    int               rc;
    ks.n = n;
    // key bits of the order; whether the record can hold them beside the position
    uint32_t K = ks.kbits, pdrop = 0;
    if (n >= 3) {
        uint32_t idbits = 1;
        while (idbits < 40 && (1ull << idbits) < ids_global + 1) ++idbits;
        K = std::max(idbits + ks.clsbits, 17u + ks.w);
        if (K - 8 + ks.posbits > 64) pdrop = 3;
        if (K - 8 + ks.posbits - pdrop > 64 || K > 48u + ks.w || (pdrop && b.pshift + 3 > ks.posbits))
            return fail(c, COLIBRI_ERR_OVERFLOW, "key-sharded pass of order %d: %u key bits and %u position bits do not fit a record", n, K, ks.posbits);
    }
    const uint32_t bsh = ks2_bshift(est_records, ks.world, K, ks.w);
    Bi2State* const       bs   = n == 2 ? c->b2.state.p : (n & 1) ? c->b2.state2.p : c->b2.state3.p;
    const Bi2State* const prev = n == 3 ? c->b2.state.p : (n & 1) ? c->b2.state3.p : c->b2.state2.p;
    auto* const           recsA = reinterpret_cast<unsigned long long*>(c->recs[0].p);
    auto* const           recsB = reinterpret_cast<unsigned long long*>(c->recs[1].p);
    ks.src_state = bs;
    HIP_TRY(c, hipMemsetAsync(bs, 0, sizeof(Bi2State), c->stream));
    HIP_TRY(c, hipMemsetAsync(ks.ks2.p, 0, sizeof(Ks2State), c->stream));
    hipLaunchKernelGGL(ks2_set_kernel, dim3(1), dim3(1), 0, c->stream, bs, ks.w, bsh);
    if (n == 2) {
        Prof p(c, COLIBRI_K_EMIT2);
        hipLaunchKernelGGL(bi2_emit_kernel, dim3(kBi2EmitGrid), dim3(kBi2Threads), 0, c->stream, c->cls.p, c->uni_surv.p, ks.nclasses / 32 + 1, npos, ks.clsbits, 0u, 0u, ks.posbits, recsA, b.region,
                           kBi2SubWide, bs, c->state.p, c->b2.head_rows.p, (uint8_t*)nullptr, ks.kbits, (more || ks.indexed) ? c->b2.plist.p : (uint32_t*)nullptr,
                           (more || ks.indexed) ? c->b2.pcode.p : (uint32_t*)nullptr, b.pl);
        hipLaunchKernelGGL(bi2_head_reduce_kernel, dim3(kBi2HeadN / kBlock, kBi2HeadSplit), dim3(kBlock), 0, c->stream, c->b2.head_rows.p, kBi2EmitGrid, bs, c->state.p);
        hipLaunchKernelGGL(ks_head_pack_kernel, dim3(kBi2HeadN / kBlock), dim3(kBlock), 0, c->stream, (const Bi2State*)bs, (uint32_t)ks.rank, ks.headg.p);
        *head_dev = ks.headg.p;
    } else {
        Prof           p(c, COLIBRI_K_EMIT);
        const uint32_t cap = chain_steps_cap(b.pl);
        hipLaunchKernelGGL(chain_steps_kernel, dim3(kChXcds), dim3(kBi2Threads), 0, c->stream, prev, b.pl, b.nbuckets, reinterpret_cast<uint2*>(c->b2.steps.p), cap,
                           c->b2.steps.p + 2 * (size_t)kChXcds * cap, (const DevState*)c->state.p);
        hipLaunchKernelGGL(chain_bits_lds(b.pl) ? chain_emit_kernel<true> : chain_emit_kernel<false>, dim3(768), dim3(kChThreads), 0, c->stream, (const uint32_t*)c->cls.p, npos, (uint32_t)n, ks.clsbits, ks.posbits - pdrop, prev,
                           (const uint32_t*)c->b2.plist.p, (const uint32_t*)c->b2.pcode.p, b.pl, reinterpret_cast<const uint2*>(c->b2.steps.p), cap,
                           (const uint32_t*)(c->b2.steps.p + 2 * (size_t)kChXcds * cap), (const uint32_t*)c->b2.bitmap.p, recsA, b.region, kBi2SubWide, bs, c->state.p,
                           (const uint32_t*)c->b2.headid.p, 0u, K, pdrop);
        *head_dev = nullptr;
    }
    {
        Prof p(c, COLIBRI_K_LEVELB2);
        // (records per A bin, scan, B-bin shift: the emit kernel's last block, bi2_offsets_tail)
        hipLaunchKernelGGL(bi2_levelB_kernel<true>, dim3(b.nslots), dim3(kBi2Threads), 0, c->stream, (const unsigned long long*)recsA, recsB, b.region, (const Bi2State*)bs, c->b2.boff.p,
                           (const DevState*)c->state.p, (const uint32_t*)nullptr, ks.cbhist.p);
    }
    {
        Prof p(c, COLIBRI_K_SCATTER);
        hipLaunchKernelGGL(ks2_hist_kernel, dim3(kBins), dim3(kKsThreads), 0, c->stream, (const uint32_t*)ks.cbhist.p, b.region, (const Bi2State*)bs, ks.w, kBi2SubWide, ks.tab.p, ks.ks2.p);
        hipLaunchKernelGGL(ks2_rows_kernel, dim3(1), dim3(kKsThreads), 0, c->stream, ks.ks2.p, (uint32_t)ks.world, (const DevState*)c->state.p, ks.small.p);
        if ((rc = ks_peek_begin(c)) || (rc = ks_peek(c, 0, ks.ks2.p->dbase, (kKsWorld + 2) * sizeof(uint32_t))) || (rc = ks_peek(c, 12, &c->state.p->radix_overflow, sizeof(uint32_t))) ||
            (rc = ks_peek(c, 13, &bs->overflow, sizeof(uint32_t))) || (rc = ks_peek(c, 14, ks.small.p, sizeof(uint32_t))))
            return rc;
        static const bool move_per_abin = getenv("COLIBRI_KS2_MOVE_ABIN") != nullptr;  // (round 4's form: a block per A bin; for comparison)
        if (move_per_abin)
            hipLaunchKernelGGL(ks2_move_kernel, dim3(kBins), dim3(kKsThreads), 0, c->stream, (const unsigned long long*)recsB, b.region, (const Bi2State*)bs, ks.w, kBi2SubWide,
                               (const uint32_t*)ks.tab.p, (const Ks2State*)ks.ks2.p, (const uint32_t*)c->b2.boff.p, b.pshift, pdrop, ks.key4.p, ks.posbuf.p);
        else
            hipLaunchKernelGGL(ks2_move_slot_kernel, dim3(kBins * kBi2SubWide), dim3(kKsThreads), 0, c->stream, (const unsigned long long*)recsB, b.region, (const Bi2State*)bs, ks.w,
                               kBi2SubWide, (const uint32_t*)ks.tab.p, (const Ks2State*)ks.ks2.p, (const uint32_t*)ks.cbhist.p, b.pshift, pdrop, ks.key4.p, ks.posbuf.p);
    }
    // the sizes were final when the rows were placed: the host reads them while the move kernel runs (the exchange is enqueued behind it)
    if ((rc = ks_peek_end(c))) return rc;
    const uint32_t* const h = ks.pinned;
    if (ks.pending_uni) {  // the unigrams kept (order 1 ran before this point of the stream)
        uint32_t kept1 = 0;
        HIP_TRY(c, hipMemcpyAsync(&kept1, &ks.stats.p->kept[1], sizeof kept1, hipMemcpyDeviceToHost, ks.side));
        HIP_TRY(c, hipStreamSynchronize(ks.side));
        ks.pending_uni = false;
        if (ks.rank == 0) {
            if (kept1) c->segments.push_back({0u, kept1, 1, kMaskFromClass});
            ks.fin_total = kept1;
        }
    }
    if (h[kKsWorld + 1] || h[12] || h[13])
        return fail(c, COLIBRI_ERR_OVERFLOW, "key-sharded pass of order %d: a record region of the emit kernel or a position list overflowed (%u / %u / %u)", n, h[kKsWorld + 1], h[12], h[13]);
    for (int d = 0; d <= kKsWorld; ++d) ks.sbase[d] = h[std::min(d, ks.world)];
    for (int d = 0; d < ks.world; ++d) per_owner[d] = h[d + 1] - h[d];
    ks.bshift  = bsh;
    *admitted  = h[14];
    *send_dev  = ks.key4.p;
    *tab_dev   = ks.tab.p;
    *tab_words = kKs2Bins;
    *recbytes  = 4;
    return COLIBRI_OK;
}

// where the caller receives the keys (the sources' streams one after the other, in rank order) and the tables (row s from rank s, *tab_words words each)
int colibri_kshard_recv_buffers(colibri_ctx* c, uint64_t nrecords, void** recv_dev, void** tab_recv_dev) {
    if (!c || !recv_dev || !tab_recv_dev) return COLIBRI_ERR_ARG;
    auto& ks = c->ks;
    if (!ks.active || ks.n < 2) return fail(c, COLIBRI_ERR_STATE, "colibri_kshard_recv_buffers out of order");
    if (nrecords >= 0x7FFFFF00ull) return fail(c, COLIBRI_ERR_OVERFLOW, "too many records for one owner");
    HIP_TRY(c, hipSetDevice(c->device));
    int rc;
    if ((rc = ks_bytes(c, ks.rbuf[0], (nrecords + 64) * 4))) return rc;
    *recv_dev     = ks.rbuf[0].p;
    *tab_recv_dev = ks.tab_recv.p;
    return COLIBRI_OK;
}

// order n >= 2, owner side: the received streams ARE the final bins (eight runs each, one per source): count, threshold on the global counts, then what goes back.
// per_src[s]: keys received from rank s. On return (one look-up):
//   *fb_dev / fb_per_dst (4-byte words)   feedback, per source in the order it sent: one bit per record, then the dense numbers of the surviving windows' keys;
//                                         nothing when n is the last order (more == 0)
//   *ex_dev / ex_per_dst                  (index in the exporter's stream | count << 32), 8 bytes: the patterns each rank exports
//   *kept_bins                            the keys this owner kept (without order 2's head): the caller gathers them, owner d's numbers are shifted by the sum before d
int colibri_kshard_count(colibri_ctx* c, int n, const uint64_t* per_src, int more, void** fb_dev, uint64_t* fb_per_dst, uint32_t* fb_bytes, void** ex_dev, uint64_t* ex_per_dst,
                         uint64_t* kept_bins) {
    if (!c || !per_src || !fb_dev || !fb_per_dst || !fb_bytes || !ex_dev || !ex_per_dst || !kept_bins) return COLIBRI_ERR_ARG;
    auto& ks = c->ks;
    if (!ks.active || n != ks.n || n < 2) return fail(c, COLIBRI_ERR_STATE, "colibri_kshard_count out of order");
    HIP_TRY(c, hipSetDevice(c->device));
    KsBases  kb{};
    Ks2Segs  sg{};
    uint64_t tot = 0;
    uint32_t ntiles = 0;
    for (int s = 0; s <= kKsWorld; ++s) {
        if (s < kKsWorld) kb.rbase[s] = (uint32_t)tot;
        sg.base[s]  = (uint32_t)tot;
        sg.tbase[s] = ntiles;
        if (s < ks.world) {
            tot += per_src[s];
            ntiles += blocks_for(per_src[s], kKs2Tile);
        }
    }
    if (tot >= 0x7FFFFF00ull) return fail(c, COLIBRI_ERR_OVERFLOW, "too many records for one owner");
    const uint32_t nrec = (uint32_t)tot, thr = (uint32_t)c->opt.mintokens;
    const uint32_t rescap = nrec + 2 * (uint32_t)kBi2HeadN;
    int            rc;
    if ((rc = ks_bytes(c, ks.osp_rep, (uint64_t)nrec + 64)) || (rc = ks_bytes(c, ks.osp_cnt, (uint64_t)nrec + 64)) || (rc = ks_bytes(c, ks.ores_rep, rescap)) ||
        (rc = ks_bytes(c, ks.ores_cnt, rescap)) || (rc = ks_bytes(c, ks.exs, (uint64_t)rescap * 8)) || (rc = ks_bytes(c, ks.code_at, (uint64_t)nrec + 64)) ||
        (rc = ks_bytes(c, ks.tcnt, (uint64_t)ntiles + 8)) || (rc = ks_bytes(c, ks.fbs, ((uint64_t)nrec + nrec / 32 + 64) * 4)))
        return rc;
    const uint32_t nl_ex = blocks_for(rescap, kKsRouteLen);
    if ((rc = ks_bytes(c, ks.lcnt, 2 * ((uint64_t)nl_ex * kKsWorld + 64))) || (rc = ks_bytes(c, ks.loff, 2 * ((uint64_t)nl_ex * kKsWorld + 64)))) return rc;
    DevState* const ost = ks.ostate.p;
    Bi2State* const obs = ks.obs.p;
    auto* const     R   = reinterpret_cast<const unsigned long long*>(ks.rbuf[0].p);  // (4-byte keys: the count kernels' KEY4 form)
    if (ks.indexed) more = 1;  // an indexed model wants every order's surviving windows back (they are its references), the last order's too
    const uint32_t* const headg = n == 2 ? (const uint32_t*)ks.headg.p : (const uint32_t*)ks.zero8k.p;
    HIP_TRY(c, hipMemsetAsync(obs, 0, sizeof(Bi2State), c->stream));
    {
        Prof p(c, COLIBRI_K_LEVELB2);
        hipLaunchKernelGGL(ks2_owner_rows_kernel, dim3(kBins), dim3(kBi2BBins), 0, c->stream, (const uint32_t*)ks.tab_recv.p, (uint32_t)ks.world, ks.oboff.p, ks.rowtot.p);
        hipLaunchKernelGGL(ks2_owner_init_kernel, dim3(1), dim3(kKsThreads), 0, c->stream, obs, ks.slotbase.p, (const uint32_t*)ks.rowtot.p, kb, ks.bshift);
        hipLaunchKernelGGL(bi2_offsets_kernel, dim3(1), dim3(kBlock), 0, c->stream, obs, 0xFFFFFFFFu, (uint32_t)kKsWorld, (const DevState*)ost);
        hipLaunchKernelGGL(bi2_binoff_kernel, dim3(kBins), dim3(kBi2BBins), 0, c->stream, obs, (const uint32_t*)ks.oboff.p, (uint32_t)kKsWorld, (const DevState*)ost);
    }
    {
        Prof p(c, COLIBRI_K_COUNT2);
        // (the hot bins' workgroups beside the wave kernel, on the second stream: they touch other bins and other records' codes)
        HIP_TRY(c, hipEventRecord(c->b2.ev_fork, c->stream));
        HIP_TRY(c, hipStreamWaitEvent(c->b2.aux, c->b2.ev_fork, 0));
        hipLaunchKernelGGL((bi2_count_big_kernel<(int)kKsWorld, true, true>), dim3(kBi2Waves * kWave / kBi2BigThreads), dim3(kBi2BigThreads), 0, c->b2.aux, R, 0u, (const uint32_t*)ks.oboff.p, obs, ost,
                           thr, ks.osp_rep.p, ks.osp_cnt.p, ks.code_at.p, (uint32_t*)nullptr, 0u, more != 0, (uint32_t*)nullptr, (const uint32_t*)ks.slotbase.p);
        HIP_TRY(c, hipEventRecord(c->b2.ev_join, c->b2.aux));
        hipLaunchKernelGGL((bi2_count_kernel<(int)kKsWorld, true, 16, true>), dim3(kBi2Waves), dim3(kWave), 0, c->stream, R, 0u, (const uint32_t*)ks.oboff.p, obs, ost, thr, ks.osp_rep.p,
                           ks.osp_cnt.p, ks.code_at.p, (uint32_t*)nullptr, 0u, more != 0, (uint32_t*)nullptr, (const uint32_t*)ks.slotbase.p, true, bi2_tail());
        HIP_TRY(c, hipStreamWaitEvent(c->stream, c->b2.ev_join, 0));
    }
    {
        Prof p(c, COLIBRI_K_PRUNE);
        hipLaunchKernelGGL(bi2_kept_scan_kernel, dim3(kBins), dim3(kBi2BBins), 0, c->stream, obs, (const DevState*)ost);
        hipLaunchKernelGGL(ks_finish2_kernel, dim3(1), dim3(kBlock), 0, c->stream, ost, obs, headg, (uint32_t)ks.rank, thr, rescap, c->b2.headsurv.p);
        hipLaunchKernelGGL(ks2_compact_kernel, dim3(1025), dim3(kBlock), 0, c->stream, (const uint32_t*)ks.osp_rep.p, (const uint32_t*)ks.osp_cnt.p, (const Bi2State*)obs,
                           (const Bi2State*)c->b2.state.p, headg, kb, (uint32_t)ks.world, ks.ores_rep.p, ks.ores_cnt.p, rescap);
        const Ks2RouteExports exsp{ks.ores_rep.p, ks.ores_cnt.p, &ost->kept, kKsRouteLen, (uint32_t)ks.rank};
        ks_route_count(c, exsp, nl_ex, (uint32_t)ks.world, ks.rstate.p + 1, 1);
        if (more && ntiles) {
            hipLaunchKernelGGL(ks2_fb_count_kernel, dim3(std::min<uint32_t>(blocks_for(ntiles, kKsThreads / kWave), 2048u)), dim3(kKsThreads), 0, c->stream, (const uint32_t*)ks.code_at.p, sg, ntiles, ks.tcnt.p);
            hipLaunchKernelGGL(scan_tiles_kernel, dim3(1), dim3(kPairThreads), 0, c->stream, ks.tcnt.p, ntiles, ks.tcnt.p + ntiles);
        } else {
            HIP_TRY(c, hipMemsetAsync(ks.tcnt.p, 0, sizeof(uint32_t) * ((size_t)ntiles + 1), c->stream));
        }
        hipLaunchKernelGGL(ks2_fb_info_kernel, dim3(1), dim3(1), 0, c->stream, (const uint32_t*)ks.tcnt.p, sg, (uint32_t)(more ? ks.world : 0), ntiles, (const Bi2State*)obs, ks.fbinfo.p);
        if ((rc = ks_peek_begin(c)) || (rc = ks_peek(c, 0, ks.rstate.p + 1, sizeof(KsRouteState))) || (rc = ks_peek(c, 32, ost, 16 * sizeof(uint32_t))) ||
            (rc = ks_peek(c, 64, ks.fbinfo.p, sizeof(Ks2FbInfo))))
            return rc;
        ks_route_move<Ks2RouteExports, 4>(c, exsp, nl_ex, (uint32_t)ks.world, reinterpret_cast<unsigned long long*>(ks.exs.p), 1);
        if (more && ntiles)
            hipLaunchKernelGGL(ks2_fb_write_kernel, dim3(std::min<uint32_t>(blocks_for(ntiles, kKsThreads / kWave), 2048u)), dim3(kKsThreads), 0, c->stream, (const uint32_t*)ks.code_at.p, sg, ntiles, (const uint32_t*)ks.tcnt.p,
                               (const Ks2FbInfo*)ks.fbinfo.p, (const Bi2State*)obs, reinterpret_cast<uint32_t*>(ks.fbs.p));
    }
    hipLaunchKernelGGL(ks_order_end_kernel, dim3(1), dim3(1), 0, c->stream, ost, c->state.p, ks.stats.p, n, 0xFFFFFFFFu);
    if ((rc = ks_peek_end(c))) return rc;
    KsRouteState hr{};
    DevState     hs{};
    Ks2FbInfo    fi{};
    std::memcpy(&hr, ks.pinned, sizeof hr);
    std::memcpy(&hs, ks.pinned + 32, 16 * sizeof(uint32_t));
    std::memcpy(&fi, ks.pinned + 64, sizeof fi);
    if (hs.overflow || hs.radix_overflow)
        return fail(c, COLIBRI_ERR_OVERFLOW, "key-sharded pass of order %d: %s", n,
                    hs.overflow ? "owner result buffer exhausted" : hs.radix_overflow == 5 ? "a record slot overflowed" : "a final bin outgrew its LDS table");
    for (int d = 0; d < ks.world; ++d) {
        fb_per_dst[d] = more ? fi.off[d + 1] - fi.off[d] : 0;
        ex_per_dst[d] = hr.dbase[d + 1] - hr.dbase[d];
    }
    *kept_bins = fi.kept_bins;
    ks.head_windows = n == 2 ? fi.head_windows : 0u;
    *fb_dev    = ks.fbs.p;
    *fb_bytes  = 4;
    *ex_dev    = ks.exs.p;
    return COLIBRI_OK;
}

// where the caller receives the feedback (4-byte words) and the exports (each concatenated in owner order)
int colibri_kshard_head_windows(const colibri_ctx* c, uint64_t* windows) {
    if (!c || !windows) return COLIBRI_ERR_ARG;
    *windows = c->ks.head_windows;
    return COLIBRI_OK;
}
int colibri_kshard_feedback_buffers(colibri_ctx* c, uint64_t nfeedback, uint64_t nexports, void** fb_recv_dev, void** ex_recv_dev) {
    if (!c || !fb_recv_dev || !ex_recv_dev) return COLIBRI_ERR_ARG;
    auto& ks = c->ks;
    if (!ks.active || ks.n < 2) return fail(c, COLIBRI_ERR_STATE, "colibri_kshard_feedback_buffers out of order");
    if (nfeedback >= 0x7FFFFF00ull || nexports >= 0x7FFFFF00ull) return fail(c, COLIBRI_ERR_OVERFLOW, "too much feedback for one rank");
    HIP_TRY(c, hipSetDevice(c->device));
    int rc;
    if ((rc = ks_bytes(c, ks.fbr, (nfeedback + 64) * 4)) || (rc = ks_bytes(c, ks.exr, (nexports + 64) * 8))) return rc;
    *fb_recv_dev = ks.fbr.p;
    *ex_recv_dev = ks.exr.p;
    return COLIBRI_OK;
}

// order n >= 2, source side again. fb_src[d] / ex_src[d]: words of feedback / exports received from owner d; kept_per_owner[d]: what owner d kept at this order
// (colibri_kshard_count's *kept_bins, gathered by the caller). The feedback becomes (position, global number) pairs of the surviving windows, sorted into position
// buckets, and the bitmap — what the next order's scan walks; the exports join this rank's share of the model. Nothing is read back.
// *ids_global: the numbers this order handed out over all ranks (the next colibri_kshard_emit wants them)
int colibri_kshard_apply(colibri_ctx* c, int n, const uint64_t* fb_src, const uint64_t* ex_src, const uint64_t* kept_per_owner, int more, uint64_t* ids_global) {
    if (!c || !fb_src || !ex_src || !kept_per_owner || !ids_global) return COLIBRI_ERR_ARG;
    auto& ks = c->ks;
    if (!ks.active || n != ks.n || n < 2) return fail(c, COLIBRI_ERR_STATE, "colibri_kshard_apply out of order");
    HIP_TRY(c, hipSetDevice(c->device));
    const uint32_t    npos = c->npos;
    const Bigram2Plan b    = bigram2_plan(c, npos);
    int               rc;
    Ks2Segs  sg{}, exs{};
    Ks2Secs  sc{};
    uint64_t nflat = 0, nex = 0, off = 0, gb = 0;
    uint32_t ntiles = 0;
    for (int d = 0; d <= kKsWorld; ++d) {
        sg.base[d]  = ks.sbase[d];
        sg.tbase[d] = ntiles;
        exs.base[d] = (uint32_t)nex;
        sc.off[d]   = (uint32_t)off;
        if (d < kKsWorld) sc.gbase[d] = (uint32_t)gb;
        if (d < ks.world) {
            const uint32_t nd = ks.sbase[d + 1] - ks.sbase[d], nwords = (nd + 31) / 32;
            ntiles += blocks_for(nd, kKs2Tile);
            if (more || ks.indexed) {
                if (fb_src[d] < nwords) return fail(c, COLIBRI_ERR_STATE, "colibri_kshard_apply: owner %d sent %llu words of feedback for %u records", d, (unsigned long long)fb_src[d], nd);
                nflat += fb_src[d] - nwords;
                off += fb_src[d];
            }
            nex += ex_src[d];
            gb += kept_per_owner[d];
        }
    }
    uint64_t nhead = 0;
    if (n == 2) {  // the head pairs' numbers lie behind all owners'; how many of them survived: the same bits on every rank (ks_finish2_kernel), counted here
        std::vector<uint32_t> hs(kBi2HeadN / 32);
        HIP_TRY(c, hipMemcpyAsync(hs.data(), c->b2.headsurv.p, sizeof(uint32_t) * hs.size(), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        ++ks.syncs;
        for (uint32_t x : hs) nhead += (uint64_t)__builtin_popcount(x);
    }
    *ids_global = gb + nhead;
    if (nflat >= 0x7FFFFF00ull || gb + nhead >= 0xFFFFFF00ull) return fail(c, COLIBRI_ERR_OVERFLOW, "key-sharded pass of order %d: too many survivors", n);
    const bool fb = more || ks.indexed;  // (the feedback of an indexed model's last order only feeds its references)
    if (fb && ks.indexed) {
        if ((uint64_t)ks.gid_off + gb + nhead >= 0x7FFFFFF0ull) return fail(c, COLIBRI_ERR_OVERFLOW, "key-sharded indexed run: more than 2^31 global pattern numbers");
        HIP_TRY(c, hipMemsetAsync(c->ids[0].p, 0xFF, sizeof(uint32_t) * ((size_t)npos + 1), c->stream));
    }
    if (fb) {
        Bi2State* const bs = ks.src_state;
        if ((rc = ks_bytes(c, ks.tcnt, (uint64_t)ntiles + 8))) return rc;
        Prof p(c, COLIBRI_K_LISTS2);
        if (ntiles) {
            hipLaunchKernelGGL(ks2_dec_count_kernel, dim3(std::min<uint32_t>(blocks_for(ntiles, kKsThreads / kWave), 2048u)), dim3(kKsThreads), 0, c->stream, reinterpret_cast<const uint32_t*>(ks.fbr.p), sg, sc, ntiles, ks.tcnt.p);
            hipLaunchKernelGGL(scan_tiles_kernel, dim3(1), dim3(kPairThreads), 0, c->stream, ks.tcnt.p, ntiles, ks.tcnt.p + ntiles);
            hipLaunchKernelGGL(ks2_dec_pospart_kernel, dim3(512), dim3(kBi2Threads), 0, c->stream, reinterpret_cast<const uint32_t*>(ks.fbr.p), sg, sc, ntiles, (const uint32_t*)ks.tcnt.p,
                               (const uint32_t*)ks.posbuf.p, bs, c->state.p, c->b2.plist.p, b.pl, c->b2.pcode.p, more != 0, ks.indexed ? c->ids[0].p : (uint32_t*)nullptr, ks.gid_off);
        }
        if (n == 2) hipLaunchKernelGGL(ks2_headid_kernel, dim3(1), dim3(kBlock), 0, c->stream, (const uint32_t*)c->b2.headsurv.p, (uint32_t)gb, c->b2.headid.p);
        if (n == 2 && ks.indexed)
            hipLaunchKernelGGL(ks2_head_ids_kernel, dim3(std::min(b.nbuckets, 1024u)), dim3(kBlock), 0, c->stream, (const Bi2State*)bs, (const uint32_t*)c->b2.plist.p, (const uint32_t*)c->b2.pcode.p,
                               b.pl, b.nbuckets, (const uint32_t*)c->b2.headid.p, ks.gid_off, c->ids[0].p);
        if (more)
        hipLaunchKernelGGL(chain_bitmap_kernel, dim3(b.nbuckets), dim3(kBi2BmThreads), ((size_t)1 << b.pshift) / 8, c->stream, npos, (const Bi2State*)bs, (const uint32_t*)c->b2.plist.p, b.pl,
                           c->state.p, c->b2.bitmap.p, n == 2 ? (const uint32_t*)c->b2.pcode.p : (const uint32_t*)nullptr, n == 2 ? (const uint32_t*)c->b2.headid.p : (const uint32_t*)nullptr);
    }
    if (nex) {
        const uint64_t need = (uint64_t)ks.fin_total + nex;
        if (need >= 0x7FFFFFF0ull) return fail(c, COLIBRI_ERR_OVERFLOW, "more than 2^31 patterns exported by one rank");
        if ((rc = grow_keep(c, ks.fin_rep, need, ks.fin_total)) || (rc = grow_keep(c, ks.fin_cnt, need, ks.fin_total)) || (ks.indexed && (rc = grow_keep(c, ks.fin_gid, need, ks.fin_total))))
            return rc;
        Prof p(c, COLIBRI_K_PRUNE);
        hipLaunchKernelGGL(ks2_append_exports_kernel, dim3(stream_grid(nex)), dim3(kBlock), 0, c->stream, (const unsigned long long*)ks.exr.p, exs, sg, (const uint32_t*)ks.posbuf.p,
                           ks.fin_rep.p + ks.fin_total, ks.fin_cnt.p + ks.fin_total);
        if (ks.indexed)
            hipLaunchKernelGGL(ks2_export_gids_kernel, dim3(stream_grid(nex)), dim3(kBlock), 0, c->stream, (const uint32_t*)(ks.fin_rep.p + ks.fin_total), (uint32_t)nex,
                               (const uint32_t*)c->ids[0].p, false, ks.fin_gid.p + ks.fin_total);
        c->segments.push_back({ks.fin_total, (uint32_t)nex, n, 0u});
        ks.fin_total += (uint32_t)nex;
    }
    if (fb && ks.indexed) {  // this order's local references: (global number, position) pairs in position order (the index sort is stable)
        const TrainPlan pl = ks_plan(c);
        c->hstate.done = 0;
        if ((rc = emit_pairs(c, pl, c->ids[0].p, true))) return rc;
        ++ks.syncs;
        ks.gid_off += (uint32_t)(gb + nhead);
    }
    return COLIBRI_OK;
}

// this rank's figures per order: distinct keys / survivors among the keys it OWNS (order 1: the global figures, on rank 0 only), windows it counted as a source.
// Sums over the ranks are the model's found / kept / admitted. Arrays of COLIBRI_MAX_ORDER entries. *syncs: host look-ups of this run so far.
int colibri_kshard_local_stats(colibri_ctx* c, uint64_t* found, uint64_t* kept, uint64_t* admitted, uint32_t* syncs) {
    if (!c || !found || !kept || !admitted) return COLIBRI_ERR_ARG;
    auto& ks = c->ks;
    if (!ks.active) return fail(c, COLIBRI_ERR_STATE, "colibri_kshard_begin first");
    HIP_TRY(c, hipSetDevice(c->device));
    int rc;
    if ((rc = ks_settle_uni(c))) return rc;
    KsStats h{};
    HIP_TRY(c, hipMemcpyAsync(&h, ks.stats.p, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    ++ks.syncs;
    for (int n = 0; n < COLIBRI_MAX_ORDER; ++n) {
        found[n]    = (n == 1 && ks.rank != 0) ? 0 : h.found[n];
        kept[n]     = (n == 1 && ks.rank != 0) ? 0 : h.kept[n];
        admitted[n] = h.admitted[n];
    }
    if (syncs) *syncs = ks.syncs;
    return COLIBRI_OK;
}

int colibri_kshard_finish(colibri_ctx* c, const uint64_t* found_global, const uint64_t* kept_global, const uint64_t* admitted_global, uint64_t totaltokens_global, int maxn,
                          colibri_stats* stats_out) {
    if (!c || !found_global || !kept_global || !admitted_global) return COLIBRI_ERR_ARG;
    auto& ks = c->ks;
    if (!ks.active) return fail(c, COLIBRI_ERR_STATE, "colibri_kshard_begin first");
    HIP_TRY(c, hipSetDevice(c->device));
    int rc;
    if ((rc = ks_settle_uni(c))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    colibri_stats& s = c->stats;
    std::memset(&s, 0, sizeof s);
    s.totaltokens = totaltokens_global;
    s.nsentences  = c->nsent;
    s.npatterns   = ks.fin_total;  // patterns THIS rank exports; the model is the union over the ranks
    s.maxn        = maxn;
    s.minn        = maxn > 0 ? 1 : 0;
    for (int n = 1; n < COLIBRI_MAX_ORDER; ++n) {
        s.found[n]    = n <= maxn ? found_global[n] : 0;
        s.kept[n]     = n <= maxn ? kept_global[n] : 0;
        s.pruned[n]   = s.found[n] - s.kept[n];
        s.admitted[n] = n <= maxn ? admitted_global[n] : 0;
        s.windows[n]  = (n <= c->opt.maxlength) ? c->windows_n[n] : 0;
    }
    s.totaltypes = s.found[1];
    // this rank's share of the model becomes the context's result: the usual export calls serve it
    std::swap(c->res_rep, ks.fin_rep);
    std::swap(c->res_cnt, ks.fin_cnt);
    if (ks.indexed) {  // the exporters' global numbers and the local forward index, where the candidate exchange leaves them (colibri_shard_export_gids / _export_index)
        std::swap(c->sh.res_gid, ks.fin_gid);
        c->sh.res_total = ks.fin_total;
        c->trained      = true;
        if ((rc = shard_finish_index(c))) return rc;
        s.nrefs = c->npairs;
    }
    c->hstate.res_total = ks.fin_total;
    c->trained          = true;
    ++c->model_serial;
    c->export_ready     = false;
    c->keybytes         = 0;
    c->last_mode        = 2;
    c->last_passes      = 1;
    ks.active           = false;
    ks.ran              = true;
    collect_events(c);
    if (stats_out) *stats_out = s;
    return COLIBRI_OK;
}
