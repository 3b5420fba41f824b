// colibri_train: the training driver. One mode plan (plan_run), its buffers (alloc_run), four order loops (train_plain, train_enqueued, train_per_pass, train_seeded), the
// skipgram passes of an indexed model (train_skipgrams_*), and the retry ladder (train_retry.hpp), which colibri_train alone walks: no loop calls an attempt again.
// (included by colibri_hip.hip)

namespace {

static_assert(colibri_retry::kReasonBin == COLIBRI_FALLBACK_BIN && colibri_retry::kReasonOrder2 == COLIBRI_FALLBACK_ORDER2 && colibri_retry::kReasonSplit == COLIBRI_FALLBACK_SPLIT &&
                  colibri_retry::kReasonChain == COLIBRI_FALLBACK_CHAIN && colibri_retry::kReasonResults == COLIBRI_FALLBACK_RESULTS &&
                  colibri_retry::kReasonPairs == COLIBRI_FALLBACK_PAIRS && colibri_retry::kReasonLdsOrder == COLIBRI_FALLBACK_LDS_ORDER &&
                  COLIBRI_FALLBACK_REGION == 1 && COLIBRI_FALLBACK_IDS == 3,
              "train_retry.hpp restates the COLIBRI_FALLBACK_* values");

constexpr int kRetry = 1003;  // a loop, a skipgram pass or finalize_index met an event that the ladder decides on (Run::ev says which)

// ---- every mode decision of one attempt: conditions on the context, the options and the environment, nothing else ------------------------------------------------
struct RunMode {
    uint32_t npos = 0;
    int      maxlength = 0;
    int      backoff   = 0;   // MAXBACKOFFLENGTH where it changes anything: the orders above backoff + 1 differ
    uint32_t wthr      = 0;   // secondary word threshold (-W), 0 = none
    uint32_t thr_skip  = 0;   // what an exhaustive pass's skipgram needs
    uint32_t uni_shift = 0;   // plain run, order 1 per class: the class ranges' shift; 0: more than 4 M classes, the atomics kernel stays
    bool constrained = false; // train(..., constrainbymodel): one membership-filtered pass per length, no look-back (constrained.hpp)
    bool filtered    = false; // train(..., filter): only the windows that match the set are counted, without look-back
    bool continued   = false; // train(..., continued = true): the set is the model the run starts from
    bool seeded      = false; // train() on a loaded model, continued = false: the set is the model the run expands, with its counts (expand.hpp, train_seeded)
    bool synced      = false; // the modes that keep every order's ids: the enqueued id-keeping loop or the per-pass loop
    // -- the plain run
    bool uni_direct = false;  // order 1 counted per class id (canonical encoding, a class space small enough for a dense array; table_mode 1 / 2 force the generic kernels)
    bool big        = false;  // more tokens than one pass per order holds: an order is counted in passes over slices of its keys
    bool binned     = false;  // radix partition + LDS count; otherwise the global open-addressed table
    bool tri_cls    = false;  // three class ids in one key: order 3 is keyed by classes, order 2 leaves survivor bytes instead of ids (KeyTrigramCls)
    bool bi_cls     = false;  // ... and order 2 is keyed by classes + the order-1 survivor bitmap: no per-position order-1 ids at all
    bool bi2        = false;  // second-generation order 2 (bigram2.hpp): class-keyed, positions in up to 30 bits
    bool bi2_split  = false;  // ... in the direct split of a sliced order
    bool chain      = false;  // orders >= 3 on the same engine (chain.hpp): one pass per order (corpora a single pass holds)
    // -- the id-keeping runs
    bool radix_synced      = false;  // their n-gram passes of order >= 2 on the radix path too (result indices as ids, see bin_count's dense codes)
    bool radix_constrained = false;  // ... and so the passes of a constrained run: a member window's key is its pattern number in the constraint set
    bool uni_synced        = false;  // order 1 on the class-indexed count array
    bool bi2_synced        = false;  // order 2 on the second-generation kernels, which then also leave the bigram's result index at every position (chain_ids_kernel)
    bool chain_synced      = false;  // orders >= 3 on the chained engine: an order's (position, dense number) pairs become its ids per position
    bool enq               = false;  // the order loop ENQUEUED, as the plain run's is: the host looks once, after the last order
    bool pair_split        = false;  // the forward index's pairs travel split (id | packed position)
    bool pairs_direct      = false;  // an indexed model on the chained engine: the pairs of the orders >= 3 straight from the orders' position lists
    bool pairs2_direct     = false;  // ... and order 2's
    bool uni_pairs_direct  = false;  // ... and order 1's from the class ids: nobody reads ids[1] then
    bool skips_enqueued    = false;  // trainskipgrams' passes without a look from the host each, if their log holds them (train_skipgrams_logged)
    bool all_ids           = false;  // COLIBRI_ALL_IDS: every order's ids are built, every pass gated by them
    bool radix() const { return radix_synced || radix_constrained; }
};

RunMode plan_run(const colibri_ctx* c, const colibri_options& o) {
    RunMode        m;
    const uint32_t npos = m.npos = c->npos;
    m.maxlength   = std::min<int>(o.maxlength, COLIBRI_MAX_ORDER - 1);
    m.seeded      = c->cs.n != 0 && c->cs.seed;
    m.constrained = c->cs.n != 0 && !c->cs.continuation && !c->cs.filter && !m.seeded;
    m.filtered    = c->cs.n != 0 && c->cs.filter;
    m.continued   = c->cs.n != 0 && c->cs.continuation;
    m.backoff     = (o.maxbackofflength >= 1 && o.maxbackofflength + 1 < m.maxlength) ? o.maxbackofflength : 0;
    m.synced      = o.indexed || o.doskipgrams || o.doskipgrams_exhaustive || m.constrained || m.backoff || m.continued || m.filtered || m.seeded;
    m.wthr        = o.mintokens_unigrams > o.mintokens ? (uint32_t)o.mintokens_unigrams : 0u;
    m.thr_skip    = o.minskiptypes > 1 ? (uint32_t)o.mintokens_skipgrams : (uint32_t)o.mintokens;  // base pruneskipgrams is a no-op when MINSKIPTYPES <= 1 (patternmodel.h:2167-2186)
    m.all_ids     = getenv("COLIBRI_ALL_IDS") != nullptr;
    const bool canonical = !(c->flags & kFlagNonCanonical);
    const bool skips     = o.doskipgrams || o.doskipgrams_exhaustive;

    m.uni_direct = !m.synced && o.table_mode == 0 && canonical && c->maxclass < (1u << 28);
    m.uni_shift  = m.uni_direct ? uni_range_shift(c) : 0u;
    // a run that the second-generation order 2 could not hold (c->b2.disabled: the ladder's) repeats on the first-generation kernels
    const bool bi2_ok = m.uni_shift != 0 && c->maxclass < (1u << 21) && o.maxlength >= 2 && bigram2_fits(c, npos) && !c->b2.disabled;
    // Up to ~128 M tokens per device one pass per order does; beyond, an order is counted in passes over slices of its keys (bigram2_order / binned_order: `big`) —
    // which needs the class-keyed orders 2 and 3; otherwise (or on request) the global open-addressed table
    m.big       = c->ntokens > big_corpus_tokens();
    m.binned    = !m.synced && (o.table_mode == 2 || (o.table_mode == 0 && (!m.big || bi2_ok)));
    m.tri_cls   = m.binned && m.uni_direct && c->maxclass < (1u << 21) && o.maxlength >= 3;
    m.bi_cls    = m.tri_cls && m.uni_shift != 0;
    m.bi2       = m.binned && bi2_ok;
    m.bi2_split = m.bi2 && bigram2_split_fits(c, npos);
    m.chain     = m.bi2 && !m.big && bigram2_plan(c, npos).sbits == 0 && chain_fits_plain(npos) && o.maxlength >= 3 && !c->b2.chain_disabled && !getenv("COLIBRI_NO_CHAIN");

    m.radix_synced      = m.synced && !m.constrained && !m.seeded && o.table_mode == 0 && c->ntokens <= big_corpus_tokens();
    m.radix_constrained = m.constrained && o.table_mode == 0 && c->ntokens <= 128ull * 1000 * 1000;
    m.uni_synced        = !m.constrained && !m.seeded && o.table_mode == 0 && canonical && c->maxclass < (1u << 28);
    // one pass only, class-keyed, no word threshold (its cut of the order-1 ids comes after their references are emitted)
    m.bi2_synced = m.radix_synced && !m.continued && !m.filtered && !m.backoff && m.wthr == 0 && canonical && uni_range_shift(c) != 0 && c->maxclass < (1u << 21) && o.maxlength >= 2 &&
                   bigram2_fits(c, npos) && bigram2_plan(c, npos).sbits == 0 && !c->b2.disabled;
    // (the wide form of the chained orders serves indexed models too; the skipgram passes on the chained engine — skip_pass_chain — have no wide form)
    m.chain_synced = m.bi2_synced && (chain_fits(npos) || (chain_fits_plain(npos) && !skips)) && o.maxlength >= 3 && !c->b2.chain_disabled && !getenv("COLIBRI_NO_CHAIN") &&
                     !getenv("COLIBRI_NO_CHAIN_IDS");
    // The benchmark's id-keeping modes (indexed model, exhaustive skipgrams; class-keyed second-generation order 2, no rarer option) with the order loop enqueued: every
    // per-order quantity lives in DevState (idm_ngram_end / idm_order_end / skip_pass_end) (reference loop: include/patternmodel.h:981-1270, skipgram call site :1163-1171)
    m.enq = m.bi2_synced && !getenv("COLIBRI_SYNCED_LOOP");
    if (m.enq && o.doskipgrams_exhaustive) {  // the skipgram passes of ALL orders share one device log: a run that may reach orders with thousands of masks keeps the per-order loop
        size_t total = 0;
        for (int n = 3; n <= m.maxlength && total <= kSegLogCap; ++n) total += n > 16 ? (size_t)kSegLogCap + 1 : gap_masks(n, o.maxskips).size();
        m.enq = total <= kSegLogCap;
    }
    const PairFormat pf = o.indexed ? pair_format(c) : PairFormat{};
    m.pair_split        = o.indexed && pf.sb != 0 && pf.sb + pf.tb <= 32 && !pf.wrap && !getenv("COLIBRI_WHOLE_PAIRS");
    // The pairs of the orders >= 3 from the position lists (chain_pairs_kernel: a rank per listed position instead of a fill and two sweeps over npos ids, which cost those
    // sparse orders more than their counting). Without skipgram passes nobody reads the ids of the orders >= 3 then, and they are not built
    m.pairs_direct     = m.enq && m.chain_synced && o.indexed && pf.sb != 0 && !getenv("COLIBRI_NO_DIRECT_PAIRS");
    m.pairs2_direct    = m.pairs_direct && chain_ids_full_applies(bigram2_plan(c, npos)) && !getenv("COLIBRI_NO_DIRECT_PAIRS2");
    m.uni_pairs_direct = m.enq && o.indexed && !skips && m.maxlength >= 2 && !getenv("COLIBRI_NO_DIRECT_PAIRS");
    m.skips_enqueued   = o.doskipgrams && m.enq && o.indexed && !getenv("COLIBRI_SYNCED_SKIPS");
    return m;
}

// Who reads ids[n] (n >= 2) of an enqueued run: trainskipgrams' lists and keys (every order), emit_pairs (order 2; the higher orders unless their pairs come from the
// lists), the exhaustive passes' part ids (parts have at most maxlength - 2 tokens; their gate is the list itself: chain_alist_kernel's windows ARE the admitted ones).
// Nobody else: an order's fill + scatter (0.06 + 0.03..0.6 ms) is skipped where nobody does
bool want_ids(const RunMode& m, const colibri_options& o, int n) {
    if (!m.chain_synced || o.doskipgrams || m.all_ids) return true;
    if (o.indexed && ((n == 2 && !m.pairs2_direct) || !m.pairs_direct)) return true;
    return o.doskipgrams_exhaustive && n <= m.maxlength - 2;
}

// ---- HBM layout (sized once; nothing is allocated inside the enqueued order loops) -----------------------------------------------------------------------------------
int plan_buffers(colibri_ctx* c, const colibri_options& o, const RunMode& m, TrainPlan& pl) {
    const uint32_t npos = m.npos;
    // table: an order admits at most `npos` windows -> 1.5x slots
    const uint64_t table_slots64 = (uint64_t)npos + (npos >> 1) + 2048;
    if (table_slots64 >= 0x7FFFFFFFull) return fail(c, COLIBRI_ERR_CORPUS, "corpus shard too large for one device table");
    pl.npos        = npos;
    pl.table_slots = (uint32_t)table_slots64;
    // results: every survivor has >= MINTOKENS occurrences; at MINTOKENS = 1 every window may be its own pattern (exhaustion is reported, never silent)
    // (a seeded run keeps a key that occurs ONCE when the loaded count carries it over the threshold)
    uint64_t per_pos = (o.mintokens < 2 || m.seeded) ? (uint64_t)std::min(o.maxlength, 8) : (m.synced ? 4u : 2u);  // results per corpus position the run can produce
    if (o.mintokens < 2 && (o.doskipgrams || o.doskipgrams_exhaustive))  // threshold 1 keeps every masked form of every window as well
        for (int n = 3; n <= std::min(o.maxlength, 13); ++n) per_pos += gap_masks(n, o.maxskips).size();  // (longer orders: the run repeats with more room if they turn up)
    // the usual bound (a survivor has >= MINTOKENS occurrences, and few orders keep many) is not a bound for repetitive corpora — every distinct sentence
    // of L tokens occurring twice keeps L (L + 1) / 2 patterns per pair —: exhaustion is reported by the kernels and colibri_train repeats the run with
    // res_scale x 4 (up to one result per position and order)
    pl.res_cap = (uint32_t)std::min<uint64_t>(0x7FFFFFF0ull, (uint64_t)npos * per_pos * c->res_scale + 1024);
    pl.thr     = (uint32_t)o.mintokens;
    constexpr uint32_t kCountLdsBytes    = kCountTile * 16u + kCountLSlot * 4u + 64u;  // keyL + cntL + slotL + winL
    constexpr uint32_t kCountBlocksPerCU = (160u * 1024u / kCountLdsBytes) < 8u ? (160u * 1024u / kCountLdsBytes) : 8u;
    pl.cnt_grid = std::max<uint32_t>(1, std::min<uint32_t>(blocks_for(npos, kCountTile), 256u * kCountBlocksPerCU));  // persistent blocks: all resident
    pl.tab_grid = stream_grid(pl.table_slots);
    pl.pos_grid = stream_grid(npos);
    return COLIBRI_OK;
}

int alloc_run(colibri_ctx* c, const colibri_options& o, const RunMode& m, const TrainPlan& pl) {
    const uint32_t npos = m.npos;
    int            rc;
    if (m.uni_direct && ((rc = dev_alloc(c, c->cnt1, (size_t)c->maxclass + 2)) || (rc = dev_alloc(c, c->rep1, (size_t)c->maxclass + 2)))) return rc;
    if (m.uni_shift && (rc = uni_alloc(c))) return rc;
    if (m.tri_cls && !m.bi2 && ((rc = dev_alloc(c, c->flags_at, (size_t)npos + 1)) || (rc = dev_alloc(c, c->flag2, (size_t)npos + 4)))) return rc;
    if (o.indexed && (rc = pairs_begin(c, npos))) return rc;
    c->pair_split = m.pair_split;

    if (c->ids.size() < 2) c->ids.resize(2);
    if ((rc = dev_alloc(c, c->ids[0], (size_t)npos + 1))) return rc;
    if ((rc = dev_alloc(c, c->ids[1], (size_t)npos + 1))) return rc;
    if (m.binned || m.radix()) {
        // recs[0]: 256 fixed-capacity A-bin regions (25 % slack over a uniform split + one scatter tile each); recs[1]: exact
        if ((rc = dev_alloc(c, c->recs[0], ((size_t)npos + (npos >> 2)) / kBins * kBins + (size_t)kBins * kScatTile * 4)) ||
            (rc = dev_alloc(c, c->recs[1], std::max<size_t>((size_t)npos + 1, (size_t)kBins * kScatTile * 4))))  // (floors: a small corpus with one hot bigram still fits its slot of the order-2 records)
            return rc;
        if ((rc = dev_alloc(c, c->rep_of, (size_t)npos + 1)) || (rc = dev_alloc(c, c->ids_at, (size_t)npos + 1)) || (rc = dev_alloc(c, c->binstate, 1))) return rc;
        if ((rc = dev_alloc(c, c->alist[0], (size_t)npos + 1)) || (rc = dev_alloc(c, c->alist[1], (size_t)npos + 1)) || (rc = dev_alloc(c, c->alist_n, 2))) return rc;
        if (m.bi2 && (rc = bigram2_alloc(c, npos, m.chain, /*keep=*/true))) return rc;
    }
    if (m.bi2_synced && (rc = bigram2_alloc(c, npos, m.chain_synced, /*keep=*/true))) return rc;
    if (!m.binned && (rc = dev_alloc(c, c->table, pl.table_slots))) return rc;  // the plain radix run needs no table (a bin overflow repeats the run on the table)
    if ((rc = dev_alloc(c, c->res_rep, pl.res_cap))) return rc;
    if ((rc = dev_alloc(c, c->res_cnt, pl.res_cap))) return rc;
    if ((rc = dev_alloc(c, c->state, 1))) return rc;
    if (o.doskipgrams || o.doskipgrams_exhaustive) {
        if ((rc = dev_alloc(c, c->scratch[0], (size_t)npos + 1))) return rc;
        if ((rc = dev_alloc(c, c->scratch[1], (size_t)npos + 1))) return rc;
    }
    if (o.doskipgrams && (rc = dev_alloc(c, c->nsrc, pl.table_slots))) return rc;
    if (m.synced && (int)c->ids.size() < m.maxlength + 2) c->ids.resize(m.maxlength + 2);  // (the per-pass loop grows its per-order id arrays lazily)
    if (m.enq) {
        if (m.pairs_direct && ((rc = dev_alloc(c, c->b2.wpre, (size_t)npos / 32 + 64)) || (rc = dev_alloc(c, c->b2.btot, kBi2Buckets)))) return rc;
        const uint32_t nclasses = c->maxclass + 1;
        if ((rc = dev_alloc(c, c->cnt1, (size_t)nclasses + 1)) || (rc = dev_alloc(c, c->rep1, (size_t)nclasses + 1)) || (rc = dev_alloc(c, c->uni_resid, (size_t)nclasses + 1)) ||
            (rc = uni_alloc(c)))
            return rc;
        for (int n = 1; n <= m.maxlength; ++n)
            if ((rc = dev_alloc(c, c->ids[n], (size_t)npos + 1))) return rc;
        if (o.doskipgrams_exhaustive && (rc = dev_alloc(c, c->seglog, 4 + 5 * (size_t)kSegLogCap))) return rc;
    }
    return COLIBRI_OK;
}

// ---- what the loops share ----------------------------------------------------------------------------------------------------------------------------------------------
struct Tally {  // per order, for the passes that follow the n-gram orders (trainskipgrams) and the forward index
    std::vector<uint32_t> valid_n, adm_n, ngram_first, ngram_kept;
    uint32_t              res_total = 0;
    void                  begin(int maxlength) {
        for (auto* v : {&valid_n, &adm_n, &ngram_first, &ngram_kept}) v->assign(maxlength + 2, 0);
    }
};
struct Run {
    colibri_ctx*           c;
    const colibri_options& o;
    const RunMode&         m;
    const TrainPlan&       pl;
    colibri_stats&         s;
    Tally                  t;
    colibri_retry::Event*  ev;
    // the ladder's turn: what happened, with DevState.radix_overflow as it is now
    int retry(colibri_retry::What what, colibri_retry::Loop loop) {
        ev->what       = what;
        ev->loop       = loop;
        ev->overflow   = c->hstate.radix_overflow;
        ev->bi2_synced = m.bi2_synced;
        ev->radix      = m.radix();
        return kRetry;
    }
};

// order 1 on the class-indexed count array (kernels.hpp §2b): no hashing, no table, LDS histogram for the Zipf head
enum class UniIds { kNone, kFromBitmap, kFromCounts, kFromResults };  // the id kernel that follows: nobody reads per-position ids | survivor bit | count >= threshold | result index per class
struct Order1 {
    uint32_t        shift;        // class ranges' shift; 0: the atomics kernel (with its representatives)
    const uint32_t* rep;          // representative positions, where the atomics kernel left some and the results want them
    uint16_t*       surv;         // the surviving bitmap, if anybody reads it
    bool            count_valid;  // no id pass follows: the finish counts the positions with a survivor
    uint32_t*       resid;        // class -> result index, if anybody reads it
    uint32_t        wthr;
    UniIds          ids;
    uint32_t*       id_out;
};
int order1_by_class(colibri_ctx* c, const TrainPlan& pl, const Order1& a) {
    const uint32_t  nclasses = c->maxclass + 1;
    const uint32_t* adm      = nullptr;  // the counts are an earlier run's: the tokens it admitted
    if (a.shift) {
        // The class counts are a property of the upload: a run on a corpus that an earlier run of this context has counted (uni_cached; nothing has written cnt1 or
        // unistate since) launches neither the fills nor the counting kernels, and the finish adds the kept token count to this run's DevState
        const bool cache = uni_cache_enabled();
        if (cache && c->uni_cached && c->cnt1.p && c->cnt1.n >= nclasses && c->unistate.p) {
            adm = &c->unistate.p->admitted;
        } else {
            // no per-token global atomics: head histogram in LDS, tail partitioned into 256 class ranges and counted per range in LDS
            const int rc = uni_count_partitioned(c, a.shift, c->cnt1.p, nclasses);
            if (rc) return rc;
            c->uni_pending = cache && hipPeekAtLastError() == hipSuccess;  // (valid once the attempt has ended well: colibri_train)
        }
    } else {
        c->uni_cached = c->uni_pending = false;
        HIP_TRY(c, hipMemsetAsync(c->cnt1.p, 0, sizeof(uint32_t) * nclasses, c->stream));
        Prof p(c, COLIBRI_K_COUNT);
        hipLaunchKernelGGL(uni_count_kernel, dim3(512), dim3(kBlock), 0, c->stream, c->cls.p, pl.npos, c->cnt1.p, c->rep1.p, c->state.p);
    }
    {
        Prof p(c, COLIBRI_K_PRUNE);
        hipLaunchKernelGGL(uni_finish_kernel, dim3(stream_grid(nclasses)), dim3(kBlock), 0, c->stream, c->cnt1.p, a.rep, nclasses, pl.thr, c->state.p, c->res_rep.p, c->res_cnt.p, pl.res_cap,
                           a.surv, a.count_valid, a.resid, a.wthr, adm);
        if (a.surv != nullptr) {  // what the survivor bitmap was made from: part of the key of order 2's kept partition (bigram2_order)
            c->b2.surv_args[0] = nclasses, c->b2.surv_args[1] = pl.thr, c->b2.surv_args[2] = a.wthr;
            c->b2.surv_known   = true;
        }
    }
    if (a.ids == UniIds::kNone) return COLIBRI_OK;
    Prof p(c, COLIBRI_K_RESOLVE);
    if (a.ids == UniIds::kFromBitmap)
        hipLaunchKernelGGL(uni_ids_bitmap_kernel, dim3(pl.pos_grid), dim3(kBlock), 0, c->stream, c->cls.p, c->uni_surv.p, (nclasses + 31) / 32, a.id_out, c->state.p, pl.npos);
    else if (a.ids == UniIds::kFromCounts)
        hipLaunchKernelGGL(uni_ids_kernel, dim3(pl.pos_grid), dim3(kBlock), 0, c->stream, c->cls.p, c->cnt1.p, std::max(pl.thr, a.wthr), a.id_out, c->state.p, pl.npos);
    else
        hipLaunchKernelGGL(uni_resid_ids_kernel, dim3(pl.pos_grid), dim3(kBlock), 0, c->stream, c->cls.p, c->uni_resid.p, a.id_out, c->state.p, pl.npos);
    return COLIBRI_OK;
}

// n-gram pass of an id-keeping run on the radix path: emit -> level B -> per-bin LDS count; survivors leave as (bin, rank) codes that the resolve turns into result
// indices (= the ids the skipgram passes and the forward index work with); use_list: only the active list is walked; build_list: the pass leaves the next order's
template <class Key>
int radix_ngram_pass(colibri_ctx* c, const TrainPlan& pl, const Key& key, uint32_t* ids_out, int n, bool use_list, bool build_list, uint32_t decode_base) {
    int rc;
    if ((rc = binned_count_stage(c, pl, key, n, use_list, pl.thr, false, true, false, /*dense_code=*/true))) return rc;
    const BinnedIO io = binned_planes(c, pl, false);
    {
        Prof p(c, COLIBRI_K_PRUNE);
        hipLaunchKernelGGL(bin_kept_scan_kernel, dim3(kBins), dim3(kBlock), 0, c->stream, c->state.p, c->binstate.p, pl.res_cap);
        hipLaunchKernelGGL(compact_bins_kernel, dim3(1024), dim3(kBlock), 0, c->stream, io.sp_rep, io.sp_cnt, c->state.p, c->binstate.p, c->res_rep.p, c->res_cnt.p, pl.res_cap,
                           use_list ? (const uint32_t*)c->alist[n & 1].p : (const uint32_t*)nullptr);
        hipLaunchKernelGGL(bin_advance_prepare_kernel, dim3(1), dim3(1), 0, c->stream, c->state.p, c->binstate.p);
    }
    return binned_resolve_stage(c, pl, ids_out, n, use_list, build_list, nullptr, 0u, /*prefill_ids=*/true, /*decode=*/true, decode_base);
}

// the first `nlogged` entries of a read-back skipgram log (skip_pass_end_kernel: result offset, kept, order, mask, found) into the figures and the result segments;
// order: only that order's entries (0: all, each under its own)
void fold_seglog(colibri_ctx* c, colibri_stats& s, const std::vector<uint32_t>& log, size_t nlogged, int order) {
    for (size_t e = 0; e < nlogged && e < log[0]; ++e) {
        const uint32_t* x = log.data() + 4 + 5 * e;
        if (order && (int)x[2] != order) continue;
        s.found[x[2]] += x[4];
        s.kept[x[2]] += x[1];
        if (x[1]) c->segments.push_back({x[0], x[1], (int)x[2], x[3]});
    }
}

// the enqueued loops peek at the termination flag only every 8 orders (MAXLENGTH defaults to 100)
int peek_done(colibri_ctx* c, int n, int maxlength, bool* done) {
    *done = false;
    if ((n % 8) != 0 || n >= maxlength) return COLIBRI_OK;
    uint32_t flag = 0;
    HIP_TRY(c, hipMemcpyAsync(&flag, &c->state.p->done, sizeof flag, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    *done = flag != 0;
    return COLIBRI_OK;
}

// ---- the headline path: all orders enqueued back to back, no host round trip per order ---------------------------------------------------------------------------------
enum class PlainEngine {
    kOrder1ByClass, kUnigram, kBigram2Chain, kChain, kBigram2Split, kBigram2, kTrigramListedSplit, kTrigramListed, kBigramCls, kBigramFlags, kTrigramCls, kNgramSplit, kNgram, kTable
};
PlainEngine plain_engine(const RunMode& m, int n, uint32_t sbits_next) {
    if (n == 1 && m.uni_direct) return PlainEngine::kOrder1ByClass;
    if (!m.binned) return PlainEngine::kTable;
    if (n == 1) return PlainEngine::kUnigram;
    if (n == 2 && m.chain) return PlainEngine::kBigram2Chain;
    if (n >= 3 && m.chain) return PlainEngine::kChain;
    if (n == 2 && m.bi2) return m.bi2_split ? PlainEngine::kBigram2Split : PlainEngine::kBigram2;
    if (n == 3 && m.bi2) return binned_split_fits(sbits_next) ? PlainEngine::kTrigramListedSplit : PlainEngine::kTrigramListed;  // over the list bigram2 left: every listed window is admissible
    if (n == 2 && m.bi_cls) return PlainEngine::kBigramCls;
    if (n == 2 && m.tri_cls) return PlainEngine::kBigramFlags;  // order 3 will not read order-2 ids
    if (n == 3 && m.tri_cls) return PlainEngine::kTrigramCls;
    if (n >= 3 && binned_split_fits(sbits_next)) return PlainEngine::kNgramSplit;
    return PlainEngine::kNgram;
}

int train_plain(Run& r) {
    auto& [c, o, m, pl, s, t, ev] = r;
    const uint32_t     npos = m.npos;
    const int          maxlength = m.maxlength;
    int                rc  = COLIBRI_OK;
    int                cur = 0;         // ids[cur] = survivor ids of order n-1; ids[cur^1] receives order n
    uint32_t           sbits_next = 0;  // passes (as a power of two) of the next first-generation order: more than one only for corpora beyond ~128 M tokens
    for (int n = 1; n <= maxlength; ++n) {
        uint32_t* id_prev = c->ids[cur].p;
        uint32_t* id_cur  = c->ids[cur ^ 1].p;
        const bool more   = n < maxlength;
        // binned orders 1-2 scan every position (almost all are admissible); from order 3 on only the positions that still carry a survivor id are visited (the
        // active list the previous order's resolve left behind)
        switch (plain_engine(m, n, sbits_next)) {
        case PlainEngine::kOrder1ByClass: {
            const bool no_ids = m.bi_cls || m.bi2;  // with class-keyed orders 2 and 3 nothing reads order-1 ids per position
            rc = order1_by_class(c, pl, {m.uni_shift, m.uni_shift ? (const uint32_t*)nullptr : c->rep1.p, m.uni_shift ? reinterpret_cast<uint16_t*>(c->uni_surv.p) : (uint16_t*)nullptr, no_ids,
                                         nullptr, m.wthr, no_ids ? UniIds::kNone : m.uni_shift ? UniIds::kFromBitmap : UniIds::kFromCounts, id_cur});
            break;
        }
        case PlainEngine::kUnigram: rc = binned_order(c, pl, KeyUnigram{c->bytes.p, c->tokstart.p}, id_cur, n, false, more); break;
        case PlainEngine::kBigram2Chain: rc = bigram2_order(c, pl, /*want_list=*/more, nullptr, /*chain=*/true); break;
        case PlainEngine::kChain: rc = chain_order(c, pl, n, /*want_next=*/more); break;
        case PlainEngine::kBigram2Split: rc = bigram2_order_split(c, pl, /*want_list=*/more); break;
        case PlainEngine::kBigram2: rc = bigram2_order(c, pl, /*want_list=*/more); break;
        case PlainEngine::kTrigramListedSplit: rc = binned_order_split(c, pl, KeyTrigramClsListed{c->cls.p}, id_cur, n, more, /*prefill_ids=*/true, sbits_next); break;
        case PlainEngine::kTrigramListed: rc = binned_order(c, pl, KeyTrigramClsListed{c->cls.p}, id_cur, n, true, more, false, /*prefill_ids=*/true, sbits_next); break;
        case PlainEngine::kBigramCls: rc = binned_order(c, pl, KeyBigramCls{c->cls.p, c->uni_surv.p}, id_cur, n, false, true, /*flag_mode=*/true); break;
        case PlainEngine::kBigramFlags: rc = binned_order(c, pl, KeyNgram{id_prev, n}, id_cur, n, false, true, /*flag_mode=*/true); break;
        case PlainEngine::kTrigramCls: rc = binned_order(c, pl, KeyTrigramCls{c->cls.p, c->flag2.p}, id_cur, n, true, more); break;
        case PlainEngine::kNgramSplit: rc = binned_order_split(c, pl, KeyNgram{id_prev, n}, id_cur, n, more, false, sbits_next); break;
        case PlainEngine::kNgram: rc = binned_order(c, pl, KeyNgram{id_prev, n}, id_cur, n, n >= 3, more, false, false, sbits_next); break;
        case PlainEngine::kTable:
            launch_clear(c, pl);
            if (n == 1)
                launch_count(c, pl, KeyUnigram{c->bytes.p, c->tokstart.p}, id_cur, 3, COLIBRI_K_COUNT);
            else
                launch_count(c, pl, KeyNgram{id_prev, n}, id_cur, 3, COLIBRI_K_COUNT);
            launch_prune(c, pl, pl.thr, nullptr, 0);
            launch_resolve(c, pl, id_cur);
            if (n == 1 && m.wthr > pl.thr) hipLaunchKernelGGL(ids_min_count_kernel, dim3(pl.pos_grid), dim3(kBlock), 0, c->stream, id_cur, c->res_cnt.p, m.wthr, npos);
            break;
        }
        if (rc) return rc;
        hipLaunchKernelGGL(advance_kernel, dim3(1), dim3(1), 0, c->stream, c->state.p, n, pl.table_slots);
        cur ^= 1;
        if (m.big && m.binned && n >= 2 && more) {  // a big corpus: how many passes the next order needs follows from how many positions still carry a survivor
            uint32_t valid = 0;
            // (after the second-generation order 2 the next order's records are exactly the entries of the list it left: windows whose two bigrams both survived)
            const uint32_t* src = (n == 2 && m.bi2) ? (const uint32_t*)(c->alist_n.p + 1) : (const uint32_t*)&c->state.p->s_valid[n];
            HIP_TRY(c, hipMemcpyAsync(&valid, src, sizeof valid, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            sbits_next = slice_bits(valid);
        }
        bool done = false;
        if ((rc = peek_done(c, n, maxlength, &done))) return rc;
        if (done) break;
    }
    if ((rc = chain_compact_join(c)) || (rc = read_state(c))) return rc;
    if (m.binned && c->hstate.radix_overflow) return r.retry(colibri_retry::What::kOverflow, colibri_retry::Loop::kPlain);
    c->last_mode   = m.binned ? 2 : 1;
    c->last_passes = m.bi2 ? (1 << bigram2_plan(c, npos).sbits) : 1;
    c->run_path    = !m.binned ? COLIBRI_PATH_TABLE
                               : (COLIBRI_PATH_RADIX | (m.bi2 ? COLIBRI_PATH_BI2 : 0) | (m.chain ? COLIBRI_PATH_CHAIN : 0) | ((m.chain && chain_wide(npos)) ? COLIBRI_PATH_WIDE : 0) |
                                  ((c->last_passes > 1 || m.big) ? COLIBRI_PATH_SLICED : 0));
    s.maxn = (int32_t)c->hstate.maxn;
    for (int n = 1; n < COLIBRI_MAX_ORDER; ++n) {
        s.found[n]    = c->hstate.s_found[n];
        s.kept[n]     = c->hstate.s_kept[n];
        s.admitted[n] = c->hstate.s_admitted[n];
        if (n <= s.maxn && s.kept[n])
            c->segments.push_back({c->hstate.res_off[n], c->hstate.res_off[n + 1] - c->hstate.res_off[n], n, (n == 1 && m.uni_shift) ? kMaskFromClass : 0u});
    }
    return COLIBRI_OK;
}

// ---- the id-keeping kinds, enqueued: the host looks once, after the last order (north star: "no host round-trip per iteration") --------------------------------------
int train_enqueued(Run& r) {
    auto& [c, o, m, pl, s, t, ev] = r;
    const uint32_t         npos = m.npos;
    const int              maxlength = m.maxlength;
    int                    rc;
    c->ids1_is_cls = !o.indexed;
    if (o.doskipgrams_exhaustive) HIP_TRY(c, hipMemsetAsync(c->seglog.p, 0, sizeof(uint32_t) * 4, c->stream));
    size_t nlogged = 0;
    for (int n = 1; n <= maxlength; ++n) {
        if (n == 1) {
            // the survivor id of a unigram is its RESULT index here, read per position through a class -> result table — unless nobody reads ids[1] (order 2 is keyed by classes)
            const bool ids1 = !c->ids1_is_cls && !m.uni_pairs_direct;
            if ((rc = order1_by_class(c, pl, {uni_range_shift(c), nullptr, reinterpret_cast<uint16_t*>(c->uni_surv.p), /*count_valid=*/!o.indexed, c->uni_resid.p, 0u,
                                              ids1 ? UniIds::kFromResults : UniIds::kNone, c->ids[1].p})))
                return rc;
            if (ids1) c->ids_built[1] = 1;
        } else if (n == 2) {
            if ((rc = bigram2_order(c, pl, /*want_list=*/true, want_ids(m, o, 2) ? c->ids[2].p : (uint32_t*)nullptr, /*chain=*/m.chain_synced))) return rc;
            c->ids_built[2] = want_ids(m, o, 2);
        } else if (m.chain_synced) {
            if (o.doskipgrams_exhaustive) {  // the windows this order admits, for its skipgram passes: from the bitmap of order n - 1, which this order's own replaces
                HIP_TRY(c, hipMemsetAsync(c->alist_n.p + (n & 1), 0, sizeof(uint32_t), c->stream));
                hipLaunchKernelGGL(chain_alist_kernel, dim3(1024), dim3(kBlock), 0, c->stream, (const uint32_t*)c->b2.bitmap.p, npos, (const DevState*)c->state.p, c->alist[n & 1].p,
                                   c->alist_n.p + (n & 1));
            }
            if ((rc = chain_order(c, pl, n, /*want_next=*/true, want_ids(m, o, n) ? c->ids[n].p : (uint32_t*)nullptr))) return rc;
            c->ids_built[(size_t)n] = want_ids(m, o, n);
            if (o.doskipgrams_exhaustive && (rc = chain_compact_join(c))) return rc;  // (the skipgram passes count in the buffers the order's survivors are being copied from)
        } else {
            if ((rc = radix_ngram_pass(c, pl, KeyNgram{c->ids[n - 1].p, n}, c->ids[n].p, n, true, true, kDecodeBaseOnDevice))) return rc;
            c->ids_built[(size_t)n] = 1;
        }
        if (n == 1 && m.uni_pairs_direct) {  // (before the order's figures are closed: the emission counts the positions with a surviving unigram, as uni_resid_ids_kernel does)
            if ((rc = emit_pairs(c, pl, c->cls.p, false, c->uni_surv.p, c->uni_resid.p, /*hot1=*/true))) return rc;
        }
        hipLaunchKernelGGL(idm_ngram_end_kernel, dim3(1), dim3(1), 0, c->stream, c->state.p, n);
        if (o.indexed && !(m.pairs_direct && (n >= 3 || (n == 2 && m.pairs2_direct))) && !(n == 1 && m.uni_pairs_direct)) {
            const uint32_t* const idn = built_ids(c, n);
            if (!idn) return COLIBRI_ERR_STATE;
            if ((rc = emit_pairs(c, pl, idn, false, nullptr, nullptr, /*hot1=*/n == 1 && !c->ids1_is_cls))) return rc;  // (ids[1] holds uni_resid's result indices then)
        }
        if (o.doskipgrams_exhaustive && n >= 3) {  // patternmodel.h:1163-1171 -> computeskipgrams :1370-1527, for every admissible window: the order's own active list
            if (n > kMaxSkipgramTokens) return fail(c, COLIBRI_ERR_UNSUPPORTED, "skipgrams of patterns longer than 31 tokens do not exist (a gap mask has 32 bits; set MAXLENGTH)");
            c->skl   = c->alist[n & 1].p;
            c->skl_n = c->alist_n.p + (n & 1);
            const std::vector<uint32_t> masks   = gap_masks(n, o.maxskips);
            const bool                  ungated = m.chain_synced && !m.all_ids;
            for (uint32_t mask : masks) {
                uint32_t f = 0, k = 0;
                const uint32_t* const gate = ungated ? (const uint32_t*)nullptr : built_ids(c, n - 1);
                if (!gate && !ungated) return COLIBRI_ERR_STATE;
                const std::vector<std::pair<int, int>> parts = mask_parts(mask, n);
                // two parts, at least one of them a single token (class id, ~20 bits; two result indices of ~24 bits do not fit a record beside the position)
                const bool one_token_part = parts.size() == 2 && c->ids1_is_cls && (parts[0].second == 1 || parts[1].second == 1);
                if (ungated && one_token_part && !o.indexed && !getenv("COLIBRI_NO_SKIP_CHAIN")) {  // ... on the chained engine
                    for (const auto& part : parts)
                        if (!(part.second == 1 && c->ids1_is_cls) && !built_ids(c, part.second)) return COLIBRI_ERR_STATE;
                    if ((rc = skip_pass_chain(c, pl, n, mask, part_ids(c, parts[0].second), (uint32_t)parts[0].first, parts[0].second == 1 && c->ids1_is_cls,
                                              part_ids(c, parts[1].second), (uint32_t)parts[1].first, parts[1].second == 1 && c->ids1_is_cls, m.thr_skip, c->seglog.p)))
                        return rc;
                    continue;
                }
                if ((rc = skipgram_pass_radix(c, pl, n, mask, gate, gate, m.thr_skip, 0u, &f, &k, nullptr, 0, 0, 0, c->seglog.p))) return rc;
            }
            nlogged += masks.size();
        }
        hipLaunchKernelGGL(idm_order_end_kernel, dim3(1), dim3(1), 0, c->stream, c->state.p, n);
        bool done = false;
        if ((rc = peek_done(c, n, maxlength, &done))) return rc;
        if (done) break;
    }
    std::vector<uint32_t> log(4 + 5 * nlogged, 0);
    if (nlogged) HIP_TRY(c, hipMemcpyAsync(log.data(), c->seglog.p, sizeof(uint32_t) * log.size(), hipMemcpyDeviceToHost, c->stream));
    if ((rc = chain_compact_join(c)) || (rc = read_state(c))) return rc;
    if (c->hstate.radix_overflow) return r.retry(colibri_retry::What::kOverflow, colibri_retry::Loop::kEnqueued);
    s.maxn = (int32_t)c->hstate.maxn;
    for (int n = 1; n <= std::min<int>(s.maxn, maxlength); ++n) {
        s.found[n]       = c->hstate.s_found[n];
        s.kept[n]        = c->hstate.s_kept[n];
        s.admitted[n]    = c->hstate.s_admitted[n];
        t.adm_n[n]       = c->hstate.s_admitted[n];
        t.valid_n[n]     = c->hstate.s_valid[n];
        t.ngram_first[n] = c->hstate.res_off[n];
        t.ngram_kept[n]  = c->hstate.s_kept[n];
        if (s.kept[n]) c->segments.push_back({c->hstate.res_off[n], c->hstate.s_kept[n], n, n == 1 ? kMaskFromClass : 0u});
        fold_seglog(c, s, log, nlogged, n);  // the order's skipgram passes, in the order they ran: their result ranges follow the n-grams'
    }
    if (s.maxn < maxlength && s.maxn + 1 < COLIBRI_MAX_ORDER) s.admitted[s.maxn + 1] = c->hstate.s_admitted[s.maxn + 1];  // (the order that found nothing still counted its windows: 0)
    t.res_total = c->hstate.res_total;
    if (c->ntokens) c->hstate.done = 0;  // (the passes that follow — skipgrams of an indexed model — write the host's copy of the state back: the loop's end is not theirs)
    return COLIBRI_OK;
}

// ---- the per-pass loop: one host round trip per pass (sizes, lazily grown per-order id arrays) --------------------------------------------------------------------------
// back-off passes (MAXBACKOFFLENGTH) and filtered runs: per-position scratch of the byte-grouping kernels
struct BackoffBufs {
    DevBuf<uint32_t>           run, flen, slot, isrep, keep;
    DevBuf<unsigned long long> off, unit, rank;
    DevBuf<FSlot>              table;
    DevBuf<FlexInfo>           info;
    DevBuf<uint8_t>            flt_cont[2];           // filtered runs: "the window at i contains a filter n-gram", this length / the one below
    DevBuf<uint32_t>           flt_exists, flt_memb;  // ... gate and result of the probes for the filter's skipgram shapes
    bool                       runs_valid = false;
};
// back-off: every window whose sub-patterns of `backoff` tokens all survived is a candidate; filtered run: every window that matches the filter is (no look-back,
// patternmodel.h:1106-1137). Either way a candidate's identity is its bytes (patternlist.hpp)
int backoff_filter_pass(Run& r, BackoffBufs& b, int n) {
    auto& [c, o, m, pl, s, t, ev] = r;
    const uint32_t     npos = m.npos;
    int                rc;
    if (!b.runs_valid) {
        if ((rc = dev_alloc(c, b.run, (size_t)npos + 1)) || (rc = dev_alloc(c, b.flen, (size_t)npos + 1)) || (rc = dev_alloc(c, b.slot, (size_t)npos + 1)) ||
            (rc = dev_alloc(c, b.isrep, (size_t)npos + 1)) || (rc = dev_alloc(c, b.keep, (size_t)npos + 1)) || (rc = dev_alloc(c, b.off, (size_t)npos + 1)) ||
            (rc = dev_alloc(c, b.unit, (size_t)npos + 1)) || (rc = dev_alloc(c, b.rank, (size_t)npos + 1)) || (rc = dev_alloc(c, b.info, 1)))
            return rc;
        if (!m.filtered) {
            Prof p(c, COLIBRI_K_COUNT);
            hipLaunchKernelGGL(backoff_runs_kernel, dim3(pl.pos_grid), dim3(kBlock), 0, c->stream, c->ids[m.backoff].p, npos, b.run.p);
        }
        b.runs_valid = true;
    }
    if (m.filtered) {  // b.run[i] = 1 where the window of n tokens at i matches the filter
        if ((rc = dev_alloc(c, b.flt_cont[0], (size_t)npos + 1)) || (rc = dev_alloc(c, b.flt_cont[1], (size_t)npos + 1)) || (rc = dev_alloc(c, b.flt_exists, (size_t)npos + 1)) ||
            (rc = dev_alloc(c, b.flt_memb, (size_t)npos + 1)))
            return rc;
        Prof p(c, COLIBRI_K_COUNT);
        const bool have_n = c->cs.has_order(n);
        if (have_n)
            hipLaunchKernelGGL(constraint_probe_kernel<false>, dim3(pl.pos_grid), dim3(kBlock), 0, c->stream, c->bytes.p, c->tokstart.p, c->cs.rem.p, c->cs.table.p, c->cs.cap,
                               c->cs.bytes.p, c->cs.off.p, npos, n, 1, c->cs.memb.p, (size_t)npos + 1, (const uint32_t*)nullptr, ~0ull);
        hipLaunchKernelGGL(filter_contains_kernel, dim3(pl.pos_grid), dim3(kBlock), 0, c->stream, c->cs.rem.p, have_n ? (const uint32_t*)c->cs.memb.p : (const uint32_t*)nullptr,
                           n > 1 ? (const uint8_t*)b.flt_cont[(n - 1) & 1].p : (const uint8_t*)nullptr, npos, (uint32_t)n, b.flt_cont[n & 1].p, b.run.p, b.flt_exists.p);
        for (const auto& shape : c->cs.shapes) {
            if (shape.first != n) continue;
            hipLaunchKernelGGL(constraint_probe_masked_kernel, dim3(pl.pos_grid), dim3(kBlock), 0, c->stream, c->bytes.p, c->tokstart.p, b.flt_exists.p, c->cs.table.p, c->cs.cap,
                               c->cs.bytes.p, c->cs.off.p, npos, n, shape.second, b.flt_memb.p);
            hipLaunchKernelGGL(filter_or_kernel, dim3(pl.pos_grid), dim3(kBlock), 0, c->stream, b.flt_memb.p, npos, b.run.p);
        }
    }
    {
        Prof p(c, COLIBRI_K_COUNT);
        hipLaunchKernelGGL(backoff_select_kernel, dim3(stream_grid((uint64_t)npos + 1)), dim3(kBlock), 0, c->stream, b.run.p, c->tokstart.p, npos, (uint32_t)n,
                           m.filtered ? 1u : (uint32_t)(n - m.backoff + 1), b.flen.p, b.off.p, b.unit.p, c->state.p);
    }
    if ((rc = read_state(c))) return rc;
    const uint32_t cand = c->hstate.admitted;
    uint32_t       kept_here = 0;
    if (cand) {
        const uint32_t cap = (uint32_t)std::min<uint64_t>(0x7FFFFFF0ull, (uint64_t)cand + (cand >> 1) + 1024);
        if ((rc = dev_alloc(c, b.table, cap))) return rc;
        bool grouped = false;
        for (int attempt = 0; attempt < 4 && !grouped; ++attempt) {
            const uint64_t seed = 0x3C6EF372FE94F82Bull + 0x9E3779B97F4A7C15ull * (uint64_t)attempt;
            HIP_TRY(c, hipMemsetAsync(b.info.p, 0, sizeof(FlexInfo), c->stream));
            {
                Prof p(c, COLIBRI_K_COUNT);
                hipLaunchKernelGGL(flex_clear_kernel, dim3(stream_grid(cap)), dim3(kBlock), 0, c->stream, b.table.p, cap);
                hipLaunchKernelGGL(flex_insert_kernel, dim3(pl.pos_grid), dim3(kBlock), 0, c->stream, c->bytes.p, b.off.p, b.flen.p, b.unit.p, npos, seed, b.table.p, cap, b.slot.p, ~0ull);
                hipLaunchKernelGGL(flex_verify_kernel, dim3(pl.pos_grid), dim3(kBlock), 0, c->stream, c->bytes.p, b.off.p, b.flen.p, npos, b.table.p, b.slot.p, b.isrep.p, b.info.p);
            }
            FlexInfo got{};
            HIP_TRY(c, hipMemcpyAsync(&got, b.info.p, sizeof got, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            HIP_TRY(c, hipGetLastError());
            grouped = !got.collision;
        }
        if (!grouped) return fail(c, COLIBRI_ERR_OVERFLOW, "back-off pass: hash collisions under four seeds");
        {
            Prof p(c, COLIBRI_K_PRUNE);
            hipLaunchKernelGGL(backoff_keep_kernel, dim3(pl.pos_grid), dim3(kBlock), 0, c->stream, b.isrep.p, b.table.p, b.slot.p, npos, pl.thr, b.keep.p, c->state.p);
        }
        unsigned long long kk = 0;
        if ((rc = scan_u32(c, b.keep.p, npos, b.rank.p, &kk))) return rc;
        kept_here = (uint32_t)kk;
        Prof p(c, COLIBRI_K_PRUNE);
        hipLaunchKernelGGL(backoff_results_kernel, dim3(pl.pos_grid), dim3(kBlock), 0, c->stream, b.keep.p, b.rank.p, b.table.p, b.slot.p, npos, r.t.res_total, pl.res_cap, c->res_rep.p,
                           c->res_cnt.p, c->state.p);
        hipLaunchKernelGGL(backoff_ids_kernel, dim3(pl.pos_grid), dim3(kBlock), 0, c->stream, b.flen.p, b.table.p, b.slot.p, npos, c->ids[n].p, c->state.p);
    } else {
        HIP_TRY(c, hipMemsetAsync(c->ids[n].p, 0xFF, sizeof(uint32_t) * (size_t)npos, c->stream));
    }
    HIP_TRY(c, hipMemcpyAsync(&c->state.p->kept, &kept_here, sizeof kept_here, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return COLIBRI_OK;
}

// one pass's results into the figures, the segments and the running total
void add_pass(Run& r, int n, uint32_t mask, uint32_t f, uint32_t k) {
    r.s.found[n] += f;
    r.s.kept[n] += k;
    if (k) r.c->segments.push_back({r.t.res_total, k, n, mask});
    r.t.res_total += k;
    r.c->hstate.res_total = r.t.res_total;
}

// the skipgram passes that belong to an order of the per-pass loop: a constrained run's, and the exhaustive ones
int skipgrams_of_order(Run& r, int n, const uint32_t* memb, bool listed_order) {
    auto& [c, o, m, pl, s, t, ev] = r;
    int                    rc;
    if (m.constrained && (o.doskipgrams || o.doskipgrams_exhaustive) && pl.thr == 1 && n >= 3) {
        // skipgrams of a constrained run: the reference reaches computeskipgrams only in its single pass at MINTOKENS = 1 (:1163: `(n >= 3) || (MINTOKENS == 1)`
        // with n == 1 in that pass); with a higher threshold a constrained run has no skipgrams at all, and neither has this one
        if (n > kMaskedMaxTokens) return fail(c, COLIBRI_ERR_UNSUPPORTED, "skipgrams of patterns longer than 13 tokens are not on the accelerated path (set MAXLENGTH)");
        for (uint32_t mask : gap_masks(n, o.maxskips)) {
            uint32_t f = 0, k = 0;
            rc = constrained_skipgram_pass(c, pl, o, n, mask, memb, m.radix_constrained, t.res_total, &f, &k);
            if (rc == kRerunOnTable) return r.retry(colibri_retry::What::kToTable, colibri_retry::Loop::kPerPass);
            if (rc) return rc;
            add_pass(r, n, mask, f, k);
        }
    } else if (!m.constrained && o.doskipgrams_exhaustive && n >= 3) {  // patternmodel.h:1163-1171 -> computeskipgrams :1370-1527, for every admissible window
        if (n > kMaxSkipgramTokens) return fail(c, COLIBRI_ERR_UNSUPPORTED, "skipgrams of patterns longer than 31 tokens do not exist (a gap mask has 32 bits; set MAXLENGTH)");
        if (m.radix_synced && listed_order) {  // the order's own active list IS the list of positions whose (n-1)-gram survived
            c->skl   = c->alist[n & 1].p;
            c->skl_n = c->alist_n.p + (n & 1);
        } else if (!built_ids(c, n - 1))
            return COLIBRI_ERR_STATE;
        else if ((rc = build_skip_list(c, pl, c->ids[n - 1].p)))
            return rc;
        const std::vector<uint32_t> masks = gap_masks(n, o.maxskips);
        const bool logged = m.radix_synced && masks.size() <= kSegLogCap;  // the order's passes are enqueued without a read-back each; one look at the log afterwards
        if (logged) {
            if ((rc = dev_alloc(c, c->seglog, 4 + 5 * (size_t)kSegLogCap))) return rc;
            HIP_TRY(c, hipMemsetAsync(c->seglog.p, 0, sizeof(uint32_t) * 4, c->stream));
            c->hstate.radix_overflow = 0;
            if ((rc = write_state(c))) return rc;  // (res_total of the orders so far; the passes advance it on the device)
        }
        for (uint32_t mask : masks) {
            uint32_t f = 0, k = 0;
            if (m.radix_synced)
                rc = skipgram_pass_radix(c, pl, n, mask, c->ids[n - 1].p, c->ids[n - 1].p, m.thr_skip, t.res_total, &f, &k, nullptr, 0, 0, 0, logged ? c->seglog.p : (uint32_t*)nullptr);
            else
                rc = skipgram_pass(c, pl, n, mask, c->ids[n - 1].p, c->ids[n - 1].p, t.adm_n[n], m.thr_skip, false, 0, &f, &k, nullptr);
            if (rc == kRerunOnTable) return r.retry(colibri_retry::What::kToTable, colibri_retry::Loop::kPerPass);
            if (rc) return rc;
            if (!logged) add_pass(r, n, mask, f, k);
        }
        if (logged && !masks.empty()) {
            std::vector<uint32_t> log(4 + 5 * masks.size());
            HIP_TRY(c, hipMemcpyAsync(log.data(), c->seglog.p, sizeof(uint32_t) * log.size(), hipMemcpyDeviceToHost, c->stream));
            if ((rc = read_state(c))) return rc;
            if (c->hstate.radix_overflow) return r.retry(colibri_retry::What::kToTable, colibri_retry::Loop::kPerPass);
            fold_seglog(c, r.s, log, masks.size(), 0);
            t.res_total = c->hstate.res_total;
        }
    }
    return COLIBRI_OK;
}

// what the per-pass loops (train_per_pass, train_seeded) share when an order has been looked at: the pass's window figures ...
void order_windows(Run& r, int n) {
    r.t.adm_n[n]    = r.c->hstate.admitted;
    r.t.valid_n[n]  = r.c->hstate.valid;
    r.s.admitted[n] = r.t.adm_n[n];
}
// ... its result segment, the running total and — an indexed model — the occurrences of its surviving n-grams (as many as positions with an id)
int close_order(Run& r, int n, uint32_t found, uint32_t kept, uint32_t mask) {
    auto& [c, o, m, pl, s, t, ev] = r;
    s.found[n] = found;
    s.kept[n]  = kept;
    if (kept) c->segments.push_back({t.res_total, kept, n, mask});
    t.ngram_first[n] = t.res_total;
    t.ngram_kept[n]  = kept;
    t.res_total += kept;
    c->hstate.res_total = t.res_total;
    return (o.indexed && kept) ? emit_pairs(c, pl, c->ids[n].p, false) : COLIBRI_OK;
}
// ... and the next order's table (at most valid_n[n] windows can be admitted: 1.5 x that many slots) and counters
int open_next_order(Run& r, int n, bool size_table) {
    auto& [c, o, m, pl, s, t, ev] = r;
    if (size_table) c->hstate.cap = (uint32_t)std::min<uint64_t>(pl.table_slots, (uint64_t)t.valid_n[n] + (t.valid_n[n] >> 1) + 1024u);
    c->hstate.found = c->hstate.kept = c->hstate.admitted = c->hstate.valid = 0;
    return write_state(c);
}

int train_per_pass(Run& r) {
    auto& [c, o, m, pl, s, t, ev] = r;
    const uint32_t         npos = m.npos;
    const int              maxlength = m.maxlength;
    int                    rc;
    bool                   list_valid = false;  // the active list of the previous radix pass exists
    if (m.constrained || m.continued || m.filtered) {
        if (!c->cs.rem_valid) {
            if ((rc = dev_alloc(c, c->cs.rem, (size_t)npos + 1))) return rc;
            hipLaunchKernelGGL(sentence_rem_kernel, dim3(stream_grid(npos)), dim3(kBlock), 0, c->stream, c->delimpos.p, c->ndelim, npos, c->cs.rem.p);
            c->cs.rem_valid = true;
        }
        // a length's distinct keys are patterns of J: the table never needs more slots than that
        c->hstate.cap = (uint32_t)std::min<uint64_t>(pl.table_slots, (uint64_t)c->cs.n + (c->cs.n >> 1) + 1024u);
        if ((rc = write_state(c))) return rc;
        if ((rc = dev_alloc(c, c->cs.memb, (size_t)(kProbeLengths + 1) * ((size_t)npos + 1)))) return rc;  // + one array: who was alive after the previous block of lengths
    }
    int         probed_from = 0, probed_to = -1;  // window lengths whose membership arrays are current
    BackoffBufs bo;
    for (int n = m.constrained ? std::max(1, o.minlength) : 1; n <= maxlength && !c->hstate.done; ++n) {
        if ((rc = dev_alloc(c, c->ids[n], (size_t)npos + 1))) return rc;
        c->ids_built[(size_t)n] = 1;  // (the per-order loop builds every order's ids)
        if (m.continued && c->cs.has_order(n)) {
            // "Skipping n-grams, already in model" (patternmodel.h:983-995): nothing is counted; the windows that ARE patterns of the loaded model get
            // the pattern's number as their survivor id, which is all the look-back of the next order asks for (:1139-1152: this->has(subngram))
            Prof p(c, COLIBRI_K_COUNT);
            hipLaunchKernelGGL(constraint_probe_kernel<false>, dim3(pl.pos_grid), dim3(kBlock), 0, c->stream, c->bytes.p, c->tokstart.p, c->cs.rem.p, c->cs.table.p, c->cs.cap,
                               c->cs.bytes.p, c->cs.off.p, npos, n, 1, c->ids[n].p, (size_t)npos + 1, (const uint32_t*)nullptr, ~0ull);
            list_valid   = false;
            t.valid_n[n] = 1;  // (not counted: the order above simply finds no candidate when there is none)
            continue;
        }
        bool       listed_order = false;  // this order walked the active list (alist[n & 1])
        const bool radix_pass = (m.radix_constrained || (m.radix_synced && n >= 2)) && !(m.backoff && n > m.backoff + 1);
        if (m.constrained && n > probed_to) {  // which pattern of the constraint set is the window at each position, for the next lengths
            probed_from = n;
            probed_to   = std::min(maxlength, n + kProbeLengths - 1);
            Prof p(c, COLIBRI_K_COUNT);
            // a prefix-closed set probed from length 1 on stops at the first miss; the last length of a block of eight tells the next block who is still alive
            const bool early = c->cs.closed && (std::max(1, o.minlength) == 1);
            if (early && probed_from > 1)
                HIP_TRY(c, hipMemcpyAsync(c->cs.memb.p + (size_t)kProbeLengths * ((size_t)npos + 1), c->cs.memb.p + (size_t)(kProbeLengths - 1) * ((size_t)npos + 1),
                                          sizeof(uint32_t) * (size_t)npos, hipMemcpyDeviceToDevice, c->stream));
            if (early)
                hipLaunchKernelGGL(constraint_probe_kernel<true>, dim3(pl.pos_grid), dim3(kBlock), 0, c->stream, c->bytes.p, c->tokstart.p, c->cs.rem.p, c->cs.table.p, c->cs.cap,
                                   c->cs.bytes.p, c->cs.off.p, npos, probed_from, probed_to - probed_from + 1, c->cs.memb.p, (size_t)npos + 1,
                                   probed_from > 1 ? (const uint32_t*)(c->cs.memb.p + (size_t)kProbeLengths * ((size_t)npos + 1)) : (const uint32_t*)nullptr, ~0ull);
            else
                hipLaunchKernelGGL(constraint_probe_kernel<false>, dim3(pl.pos_grid), dim3(kBlock), 0, c->stream, c->bytes.p, c->tokstart.p, c->cs.rem.p, c->cs.table.p, c->cs.cap,
                                   c->cs.bytes.p, c->cs.off.p, npos, probed_from, probed_to - probed_from + 1, c->cs.memb.p, (size_t)npos + 1, (const uint32_t*)nullptr, ~0ull);
        }
        const KeyMember member{c->cs.memb.p + (size_t)(m.constrained ? n - probed_from : 0) * ((size_t)npos + 1)};
        if (!(n == 1 && m.uni_synced) && !radix_pass) launch_clear(c, pl);  // only the table passes need the table cleared
        const bool backoff_pass = (m.backoff && n > m.backoff + 1) || m.filtered;
        if (backoff_pass) {
            if ((rc = backoff_filter_pass(r, bo, n))) return rc;
            list_valid = false;
        } else if (n == 1 && m.uni_synced) {
            // order 1 per class (as in the plain mode); the survivor id of a unigram is its RESULT index here, read per position through a class -> result table
            const uint32_t nclasses = c->maxclass + 1;
            const uint32_t shift    = uni_range_shift(c);
            if ((rc = dev_alloc(c, c->cnt1, (size_t)nclasses + 1)) || (rc = dev_alloc(c, c->rep1, (size_t)nclasses + 1)) || (rc = dev_alloc(c, c->uni_resid, (size_t)nclasses + 1))) return rc;
            if (shift && (rc = uni_alloc(c))) return rc;
            // per-position order-1 ids (result indices): read by the forward index and by a first-generation order 2; the skipgram passes of an unindexed run
            // name their one-token parts by class id instead (part_ids), and no id pass follows then
            c->ids1_is_cls = m.bi2_synced && !o.indexed;
            if ((rc = order1_by_class(c, pl, {shift, nullptr, m.bi2_synced ? reinterpret_cast<uint16_t*>(c->uni_surv.p) : (uint16_t*)nullptr, /*count_valid=*/c->ids1_is_cls, c->uni_resid.p, 0u,
                                              c->ids1_is_cls ? UniIds::kNone : UniIds::kFromResults, c->ids[n].p})))
                return rc;
        } else if (n == 2 && m.bi2_synced) {
            // order 2 on the second-generation kernels (bigram2.hpp), which also leave the bigrams' result indices per position and the active list of order 3
            c->hstate.radix_overflow = 0;
            if ((rc = write_state(c))) return rc;
            if ((rc = bigram2_order(c, pl, /*want_list=*/true, c->ids[n].p))) return rc;
            list_valid = true;
        } else if (radix_pass) {
            // from order 3 on only the active list is walked (a constrained pass has no look-back, hence no list: every position is asked whether its window is a member)
            const bool use_list = !m.constrained && n >= 3 && list_valid;
            listed_order        = use_list;
            c->hstate.radix_overflow = 0;
            if ((rc = write_state(c))) return rc;
            if (m.constrained)
                rc = radix_ngram_pass(c, pl, member, c->ids[n].p, n, false, false, t.res_total);
            else
                rc = radix_ngram_pass(c, pl, KeyNgram{c->ids[n - 1].p, n}, c->ids[n].p, n, use_list, true, t.res_total);
            if (rc) return rc;
            list_valid = !m.constrained;
        } else {
            if (m.constrained)
                launch_count(c, pl, member, c->ids[n].p, 3, COLIBRI_K_COUNT);
            else if (n == 1)
                launch_count(c, pl, KeyUnigram{c->bytes.p, c->tokstart.p}, c->ids[n].p, 3, COLIBRI_K_COUNT);
            else
                launch_count(c, pl, KeyNgram{c->ids[n - 1].p, n}, c->ids[n].p, 3, COLIBRI_K_COUNT);
            launch_prune(c, pl, pl.thr, nullptr, 0);
            launch_resolve(c, pl, c->ids[n].p);
        }
        if ((rc = read_state(c))) return rc;
        // (the second-generation order 2 could not hold this corpus; a bin outgrew its LDS table: the ladder knows which of the two this loop acts on)
        if (c->hstate.radix_overflow && ((m.bi2_synced && c->hstate.radix_overflow == 4) || m.radix())) return r.retry(colibri_retry::What::kOverflow, colibri_retry::Loop::kPerPass);
        const uint32_t found = c->hstate.found, kept = c->hstate.kept;
        order_windows(r, n);
        if (found == 0 && !m.constrained && !m.continued && !(m.filtered && pl.thr == 1)) break;  // "None found" (patternmodel.h:1189-1194: `if (!continued) break`); a constrained run is one pass over all lengths
        if (found) s.maxn = n;
        if ((rc = close_order(r, n, found, kept, (n == 1 && m.uni_synced && !backoff_pass) ? kMaskFromClass : 0u))) return rc;
        // secondary word threshold: the unigrams below it keep their place (and references) in the model, but take no part in longer patterns
        if (n == 1 && m.wthr > pl.thr) hipLaunchKernelGGL(ids_min_count_kernel, dim3(pl.pos_grid), dim3(kBlock), 0, c->stream, c->ids[n].p, c->res_cnt.p, m.wthr, npos);
        if ((rc = skipgrams_of_order(r, n, member.memb, listed_order))) return rc;
        if ((rc = open_next_order(r, n, !m.constrained))) return rc;
        if (t.valid_n[n] == 0 && !m.constrained && !m.continued && !m.filtered && !(m.backoff && n >= m.backoff + 1)) break;  // nothing can be admitted at n + 1 (a back-off order asks the order-b survivors instead)
    }
    return COLIBRI_OK;
}

// ---- the seeded loop: train() on a loaded model with continued = false (expand.hpp; reference include/patternmodel.h:880-1270) ---------------------------------------
// Every order on the global table: count -> seed join -> (the host looks: did the order create a key?) -> prune -> resolve -> the seeds' rows. found[n] = created keys.
int train_seeded(Run& r) {
    auto& [c, o, m, pl, s, t, ev] = r;
    auto&          cs   = c->cs;
    const uint32_t npos = m.npos;
    int            rc;
    if (!cs.rem_valid) {
        if ((rc = dev_alloc(c, cs.rem, (size_t)npos + 1))) return rc;
        hipLaunchKernelGGL(sentence_rem_kernel, dim3(stream_grid(npos)), dim3(kBlock), 0, c->stream, c->delimpos.p, c->ndelim, npos, cs.rem.p);
        cs.rem_valid = true;
    }
    // before any order: no seed occurs in a result row, every seed stays (the orders the run prunes say otherwise)
    HIP_TRY(c, hipMemsetAsync(cs.seed_slot.p, 0xFF, sizeof(uint32_t) * cs.n, c->stream));
    HIP_TRY(c, hipMemsetAsync(cs.seed_row.p, 0xFF, sizeof(uint32_t) * cs.n, c->stream));
    HIP_TRY(c, hipMemsetAsync(cs.seed_kept.p, 1, cs.n, c->stream));
    cs.seed_ran = true;
    for (int n = 1; n <= m.maxlength && !c->hstate.done; ++n) {
        if ((rc = dev_alloc(c, c->ids[n], (size_t)npos + 1))) return rc;
        c->ids_built[(size_t)n] = 1;
        HIP_TRY(c, hipMemsetAsync(cs.seed_info.p, 0, sizeof(SeedInfo), c->stream));
        launch_clear(c, pl);
        if (n == 1)
            launch_count(c, pl, KeyUnigram{c->bytes.p, c->tokstart.p}, c->ids[n].p, 3, COLIBRI_K_COUNT);
        else
            launch_count(c, pl, KeyNgram{c->ids[n - 1].p, n}, c->ids[n].p, 3, COLIBRI_K_COUNT);
        {
            Prof p(c, COLIBRI_K_JOIN);
            hipLaunchKernelGGL(seed_join_kernel, dim3(pl.tab_grid), dim3(kBlock), 0, c->stream, c->table.p, (const DevState*)c->state.p, c->bytes.p, c->tokstart.p, n, cs.table.p, cs.cap,
                               cs.bytes.p, cs.off.p, cs.seed_count.p, cs.seed_slot.p, cs.seed_info.p);
        }
        SeedInfo info{};
        HIP_TRY(c, hipMemcpyAsync(&info, cs.seed_info.p, sizeof info, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        HIP_TRY(c, hipGetLastError());
        if (info.saturated) return fail(c, COLIBRI_ERR_OVERFLOW, "expanding a loaded model: a loaded count plus the corpus' exceeds 2^32 - 1 at order %d", n);
        const bool stop = info.created == 0;  // "None found" BEFORE the prune (patternmodel.h:1189-1194): the order's counts stay, nothing of it is pruned
        launch_prune(c, pl, stop ? 0u : pl.thr, nullptr, 0);
        launch_resolve(c, pl, c->ids[n].p);
        if (cs.has_order(n)) {
            Prof p(c, COLIBRI_K_JOIN);
            hipLaunchKernelGGL(seed_rows_kernel, dim3(stream_grid(cs.n)), dim3(kBlock), 0, c->stream, cs.n, cs.seed_order.p, n, cs.seed_slot.p, cs.seed_count.p, (const Slot*)c->table.p, pl.thr,
                               stop ? 1 : 0, cs.seed_row.p, cs.seed_kept.p, cs.seed_info.p);
        }
        SeedInfo after{};  // (erased: the order's seeds that never occurred and go)
        HIP_TRY(c, hipMemcpyAsync(&after, cs.seed_info.p, sizeof after, hipMemcpyDeviceToHost, c->stream));
        if ((rc = read_state(c))) return rc;
        const uint32_t kept = c->hstate.kept;
        order_windows(r, n);
        if (!stop) s.maxn = n;
        // what prune(MINTOKENS, n) erased (patternmodel.h:1220): the order's distinct keys that were not kept, and the loaded patterns of n tokens that never occurred and
        // lie below the threshold; nothing at the order the run stopped at
        s.pruned[n] = (uint64_t)c->hstate.found - kept + after.erased;
        if ((rc = close_order(r, n, info.created, kept, 0u))) return rc;
        if (stop) break;
        // the next order's look-back: the loaded patterns of n tokens that stay although the order did not count their windows (none in a closed seed set)
        if (cs.seed_open && n >= 2 && n < m.maxlength && cs.has_order(n)) {
            {
                Prof p(c, COLIBRI_K_JOIN);
                hipLaunchKernelGGL(seed_fill_kernel, dim3(pl.pos_grid), dim3(kBlock), 0, c->stream, c->ids[n].p, cs.rem.p, npos, c->bytes.p, c->tokstart.p, n, cs.table.p, cs.cap, cs.bytes.p,
                                   cs.off.p, cs.seed_count.p, pl.thr, cs.seed_info.p);
            }
            HIP_TRY(c, hipMemcpyAsync(&info, cs.seed_info.p, sizeof info, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            HIP_TRY(c, hipGetLastError());
            t.valid_n[n] += info.filled;
        }
        if ((rc = open_next_order(r, n, true))) return rc;
        if (t.valid_n[n] == 0) break;  // nothing can be admitted at n + 1: it would create nothing and stop there, with nothing counted
    }
    if (o.indexed && t.res_total) {  // the rows' own references, for the export's offsets
        if ((rc = dev_alloc(c, c->seed_refcnt, (size_t)t.res_total))) return rc;
        HIP_TRY(c, hipMemcpyAsync(c->seed_refcnt.p, c->res_cnt.p, sizeof(uint32_t) * t.res_total, hipMemcpyDeviceToDevice, c->stream));
        hipLaunchKernelGGL(seed_refcnt_kernel, dim3(stream_grid(cs.n)), dim3(kBlock), 0, c->stream, cs.n, (const uint32_t*)cs.seed_row.p, (const uint32_t*)cs.seed_count.p, t.res_total,
                           c->seed_refcnt.p);
    }
    return COLIBRI_OK;
}

// ---- IndexedPatternModel::trainskipgrams (patternmodel.h:2969-3010): from the SURVIVING n-grams, n = 3.. ---------------------------------------------------------------
// ... enqueued, when the n-gram orders were: no look at a pass from the host — its counters, the filler filter's sizes and "None found" live on the device, one log per
// run (skip_pass_end_kernel) —; each pass used to cost two read-backs (0.9 ms of the indexed + skipgrams step in stream drains)
int train_skipgrams_logged(Run& r, int top) {
    auto& [c, o, m, pl, s, t, ev] = r;
    int                    rc;
    if ((rc = dev_alloc(c, c->seglog, 4 + 5 * (size_t)kSegLogCap))) return rc;
    HIP_TRY(c, hipMemsetAsync(c->seglog.p, 0, sizeof(uint32_t) * 4, c->stream));
    c->hstate.found = c->hstate.kept = c->hstate.admitted = c->hstate.valid = 0;
    c->hstate.radix_overflow = 0;
    c->hstate.res_total      = t.res_total;
    if ((rc = write_state(c))) return rc;
    size_t nlogged = 0;
    for (int n = 3; n <= top; ++n) {
        if (!built_ids(c, n)) return COLIBRI_ERR_STATE;
        if ((rc = build_skip_list(c, pl, c->ids[n].p))) return rc;
        const std::vector<uint32_t> masks = gap_masks(n, o.maxskips);
        const uint32_t minsrc = o.minskiptypes > 1 ? (uint32_t)o.minskiptypes : 0u;
        const uint32_t bound  = t.valid_n[n] / std::max(1u, pl.thr) + 1;  // a kept skipgram has >= MINTOKENS of the list's windows
        for (uint32_t mask : masks) {
            uint32_t  f = 0, k = 0;
            uint32_t* ids = nullptr;
            if ((rc = skipgram_pass_radix(c, pl, n, mask, c->ids[n].p, nullptr, pl.thr, 0u, &f, &k, &ids, minsrc, t.ngram_first[n], t.ngram_kept[n], c->seglog.p, bound))) return rc;
            if ((rc = emit_pairs_list(c, t.valid_n[n], ids))) return rc;  // (a pass that kept nothing left no valid id)
        }
        hipLaunchKernelGGL(skip_order_end_kernel, dim3(1), dim3(1), 0, c->stream, c->state.p, (const uint32_t*)c->seglog.p, (uint32_t)nlogged, (uint32_t)masks.size());
        nlogged += masks.size();
    }
    std::vector<uint32_t> log(4 + 5 * nlogged, 0);
    if (nlogged) HIP_TRY(c, hipMemcpyAsync(log.data(), c->seglog.p, sizeof(uint32_t) * log.size(), hipMemcpyDeviceToHost, c->stream));
    if ((rc = read_state(c))) return rc;
    if (c->hstate.radix_overflow) return r.retry(colibri_retry::What::kToTable, colibri_retry::Loop::kEnqueued);
    fold_seglog(c, r.s, log, nlogged, 0);
    t.res_total = c->hstate.res_total;
    return COLIBRI_OK;
}

int train_skipgrams_per_pass(Run& r, int top) {
    auto& [c, o, m, pl, s, t, ev] = r;
    int                    rc;
    const uint32_t         minsrc = o.minskiptypes > 1 ? (uint32_t)o.minskiptypes : 0u;
    for (int n = 3; n <= top; ++n) {
        if (n > kMaxSkipgramTokens) return fail(c, COLIBRI_ERR_UNSUPPORTED, "skipgrams of patterns longer than 31 tokens do not exist (a gap mask has 32 bits; set MAXLENGTH)");
        uint32_t found_n = 0;
        if (!built_ids(c, n)) return COLIBRI_ERR_STATE;
        if ((rc = build_skip_list(c, pl, c->ids[n].p))) return rc;
        for (uint32_t mask : gap_masks(n, o.maxskips)) {
            uint32_t f = 0, k = 0;
            int fs = 0;
            if (m.radix_synced) {
                uint32_t* ids = nullptr;
                rc = skipgram_pass_radix(c, pl, n, mask, c->ids[n].p, nullptr, pl.thr, t.res_total, &f, &k, &ids, minsrc, t.ngram_first[n], t.ngram_kept[n]);
                if (rc == kRerunOnTable) return r.retry(colibri_retry::What::kToTable, colibri_retry::Loop::kPerPass);
                if (rc) return rc;
                if (k && (rc = emit_pairs_list(c, t.valid_n[n], ids))) return rc;  // occurrences of the kept skipgrams of this pass -> forward index, over the order's list
            } else {
                if ((rc = skipgram_pass(c, pl, n, mask, c->ids[n].p, nullptr, t.valid_n[n], pl.thr, true, minsrc, &f, &k, &fs))) return rc;
                if (k) {  // occurrences of the kept skipgrams of this pass -> forward index
                    hipLaunchKernelGGL(skip_result_ids_kernel, dim3(pl.pos_grid), dim3(kBlock), 0, c->stream, c->scratch[fs].p, c->table.p, c->scratch[fs ^ 1].p, m.npos);
                    if ((rc = emit_pairs(c, pl, c->scratch[fs ^ 1].p, false))) return rc;
                }
            }
            found_n += f;
            add_pass(r, n, mask, f, k);
        }
        if (!found_n) break;  // " None found" (:2992-2994)
    }
    return COLIBRI_OK;
}

// the id-keeping kinds: their order loop, trainskipgrams, the forward index
int train_synced(Run& r) {
    auto& [c, o, m, pl, s, t, ev] = r;
    int                    rc;
    c->ids_built.assign(c->ids.size(), 0);
    c->ids1_is_cls = false;
    r.t.begin(m.maxlength);
    if ((rc = m.enq ? train_enqueued(r) : m.seeded ? train_seeded(r) : train_per_pass(r))) return rc;
    if (o.doskipgrams && !m.constrained) {
        const int top = std::min<int>(m.maxlength, r.s.maxn);
        bool      logged = false;  // (what the n-gram orders found decides whether the log holds the passes)
        if (m.skips_enqueued) {
            size_t total = 0;
            for (int n = 3; n <= top && total <= kSegLogCap; ++n) total += n > 16 ? (size_t)kSegLogCap + 1 : gap_masks(n, o.maxskips).size();
            logged = total <= kSegLogCap && top <= kMaxSkipgramTokens;
        }
        if (!logged)
            rc = train_skipgrams_per_pass(r, top);
        else if (top >= 3)
            rc = train_skipgrams_logged(r, top);
        if (rc) return rc;
    }
    c->hstate.res_total = r.t.res_total;
    c->last_mode        = m.radix() ? 2 : 1;
    c->last_passes      = 1;
    c->run_path         = !m.radix() ? COLIBRI_PATH_TABLE
                                     : (COLIBRI_PATH_RADIX | (m.bi2_synced ? COLIBRI_PATH_BI2 : 0) | (m.chain_synced ? COLIBRI_PATH_CHAIN : 0) |
                                        ((m.chain_synced && chain_wide(m.npos)) ? COLIBRI_PATH_WIDE : 0));
    if (!m.enq) c->run_path |= COLIBRI_PATH_PER_PASS;
    if (o.indexed) c->run_path |= c->pair_sb == 0 ? COLIBRI_PATH_PAIRS_UNPACKED : (!c->pair_split ? COLIBRI_PATH_PAIRS_WHOLE : 0);
    if (o.indexed && (rc = finalize_index(c, r.t.res_total))) {
        // (a model with more than two references per position; a rank that failed its check)
        if (rc == kRerunPairs || rc == kRerunRanks) return r.retry(rc == kRerunPairs ? colibri_retry::What::kPairs : colibri_retry::What::kRanks, colibri_retry::Loop::kPerPass);
        return rc;
    }
    return COLIBRI_OK;
}

// one attempt of a training run under the flags colibri_train has applied; kRetry: *ev is the ladder's
int colibri_train_once(colibri_ctx* c, const colibri_options& opt, colibri_retry::Event* ev) {
    if (!c->have_corpus) return fail(c, COLIBRI_ERR_STATE, "no corpus uploaded");
    colibri_options o = opt;
    int             rc;
    if ((rc = check_options(c, o))) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    c->opt     = o;
    c->trained = false;
    c->seeded_model = false;
    c->ks.ran  = false;
    c->profile = o.profile;
    collect_events(c);
    std::fill(std::begin(c->k_ms), std::end(c->k_ms), 0.0);
    std::fill(std::begin(c->k_launches), std::end(c->k_launches), 0);
    c->segments.clear();
    c->npairs = 0;
    c->b2.pairs_direct  = false;
    c->b2.pairs2_direct = false;
    if (c->b2.compact_pending) {  // (a run that ended early left a copy on the second stream)
        (void)hipStreamSynchronize(c->b2.aux);
        c->b2.compact_pending = false;
    }
    if (o.dopatternperline) return train_pattern_list(c, o, nullptr);

    const RunMode m = plan_run(c, o);
    TrainPlan     pl{};
    if ((rc = plan_buffers(c, o, m, pl))) return rc;
    c->res_cap_used     = pl.res_cap;
    c->b2.pairs_direct  = m.pairs_direct;
    c->b2.pairs2_direct = m.pairs2_direct;
    c->profile_class    = m.bi2 ? COLIBRI_K_COUNT2 : (m.binned || m.radix_synced) ? COLIBRI_K_BINCOUNT : COLIBRI_K_COUNT;
    if ((rc = alloc_run(c, o, m, pl))) return rc;

    // order 1: distinct unigrams <= distinct class ids when the encoding is canonical
    DevState init{};
    uint64_t cap1 = (uint64_t)c->ntokens + (c->ntokens >> 1) + 1024;
    if (!(c->flags & kFlagNonCanonical)) cap1 = std::min<uint64_t>(cap1, 2ull * ((uint64_t)c->maxclass + 1) + 1024);
    init.cap = (uint32_t)std::min<uint64_t>(cap1, pl.table_slots);
    if (c->ntokens == 0) init.done = 1;  // empty corpus: "None found" at n = 1
    c->hstate = init;
    if ((rc = write_state(c))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));

    colibri_stats& s = c->stats;
    std::memset(&s, 0, sizeof s);
    const auto t0 = std::chrono::steady_clock::now();
    Run        r{c, o, m, pl, s, Tally{}, ev};
    if ((rc = m.synced ? train_synced(r) : train_plain(r))) return rc;
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    collect_events(c);

    s.totaltokens = c->ntokens;
    s.nsentences  = c->nsent;
    s.npatterns   = c->hstate.res_total;
    s.minn        = s.npatterns ? 1 : 0;
    s.train_ms    = ms;
    for (int n = 1; n < COLIBRI_MAX_ORDER; ++n) {
        if (!m.seeded) s.pruned[n] = s.found[n] - s.kept[n];  // (a seeded run's found[n] is the keys CREATED: train_seeded has its pruned[n])
        s.windows[n] = (n <= o.maxlength) ? c->windows_n[n] : 0;
    }
    if (m.seeded) s.totaltypes = s.maxn >= 1 ? (uint64_t)c->cs.n + s.found[1] : 0;  // size() of the whole model at order 1 (patternmodel.h:1199-1201): every loaded pattern + the unigrams created
    else s.totaltypes = m.constrained ? 0 : s.found[1];  // distinct unigrams before pruning (patternmodel.h:1199-1201); a constrained run leaves it unset (:1197: constrainbymodel != NULL)
    c->trained   = true;
    c->seeded_model = m.seeded;
    ++c->model_serial;
    c->keybytes  = 0;
    c->export_ready = false;  // key lengths / offsets: computed when the results are first asked for (colibri_result_sizes), not part of counting
    s.nrefs    = o.indexed ? c->npairs : 0;
    return COLIBRI_OK;
}

// (experimental builds only) where the instrumented kernels spent their cycles, summed over the launches of one attempt
void dump_kernel_clocks() {
#ifdef BI2_PROF  // bi2_count_kernel's waves: sections of process_bin
    {
        unsigned long long h[16] = {0}, z[16] = {0};
        if (hipMemcpyFromSymbol(h, HIP_SYMBOL(colibri::bi2_prof), sizeof h) == hipSuccess) {
            unsigned long long t = 0;
            for (int k = 0; k < 12; ++k) t += h[k];
            fprintf(stderr, "BI2_PROF");
            for (int k = 0; k < 12; ++k) fprintf(stderr, " s%d=%.1f%%", k, t ? 100.0 * (double)h[k] / (double)t : 0.0);
            fprintf(stderr, " total=%llu\n", t);
            (void)hipMemcpyToSymbol(HIP_SYMBOL(colibri::bi2_prof), z, sizeof z);
        }
    }
#endif
#ifdef COLIBRI_KPROF  // phase clocks of the block-structured kernels (device_common.hpp): share of each section, summed over blocks
    {
        static const char* const names[8] = {"bi2_emit", "levelB", "uni_onepass", "pospart", "chain_emit", "hot_write", "k6", "k7"};
        unsigned long long h[8][12], z[8][12];
        memset(z, 0, sizeof z);
        if (hipMemcpyFromSymbol(h, HIP_SYMBOL(colibri::kprof), sizeof h) == hipSuccess) {
            for (int k = 0; k < 8; ++k) {
                unsigned long long t = 0;
                for (int s = 0; s < 12; ++s) t += h[k][s];
                if (!t) continue;
                fprintf(stderr, "KPROF %-12s", names[k]);
                for (int s = 0; s < 12; ++s)
                    if (h[k][s]) fprintf(stderr, " s%d=%.1f%%", s, 100.0 * (double)h[k][s] / (double)t);
                fprintf(stderr, " total=%.1fM\n", (double)t / 1e6);
            }
            (void)hipMemcpyToSymbol(HIP_SYMBOL(colibri::kprof), z, sizeof z);
        }
    }
#endif
}

// COLIBRI_DEBUG_OVERFLOW: which part of a second-generation engine gave up in the plain loop (reads memory, nothing else)
void explain_chain_overflow(colibri_ctx* c) {  // Bi2State.overflow 1 a record region / the key bits, 2 a final bin's table, 3 a position list
    uint32_t w2 = 0, w3 = 0;
    if (c->b2.state2.p) (void)hipMemcpy(&w2, &c->b2.state2.p->overflow, sizeof w2, hipMemcpyDeviceToHost);
    if (c->b2.state3.p) (void)hipMemcpy(&w3, &c->b2.state3.p->overflow, sizeof w3, hipMemcpyDeviceToHost);
    fprintf(stderr, "colibri: a chained order gave up (Bi2State.overflow of the odd / even orders now: %u / %u; first: overflow %u, key bits %u, position bits %u, bshift %u); "
                    "repeating with orders >= 3 on the first-generation kernels\n", w2, w3, c->hstate.pad[0] & 255u, (c->hstate.pad[0] >> 8) & 255u, (c->hstate.pad[0] >> 16) & 255u,
            c->hstate.pad[0] >> 24);
}
void explain_order2_overflow(colibri_ctx* c, bool small_passes) {  // 1 a record region, 2 a final bin's table, 3 a position list; 0: the position buckets or a split
    uint32_t why = 0;
    (void)hipMemcpy(&why, &c->b2.state.p->overflow, sizeof why, hipMemcpyDeviceToHost);
    fprintf(stderr, "colibri: second-generation order 2 gave up (Bi2State.overflow = %u); repeating %s\n", why, small_passes ? "with round 3's pass size" : "on the first-generation kernels");
}

}  // namespace

// A run that gives up on an engine is repeated (exactly) on the next one down or with more room: colibri_stats.fallback_reason / retries report it. The ladder
// (train_retry.hpp) says what runs next; its flags live on the context (and in tl_small_passes) for the length of one attempt
extern "C" int colibri_train(colibri_ctx* c, const colibri_options* opt_in, colibri_stats* stats_out) {
    using namespace colibri_retry;
    if (!c || !opt_in) return COLIBRI_ERR_ARG;
    c->run_path = c->run_fallback = c->run_retries = 0;
    Ladder ladder;
    int    rc;
    for (;;) {
        colibri_options o = *opt_in;
        if (ladder.attempt.force_table) o.table_mode = 1;
        if (ladder.attempt.b2_disabled) c->b2.disabled = true;
        if (ladder.attempt.chain_disabled) c->b2.chain_disabled = true;
        if (ladder.attempt.small_passes) tl_small_passes = true;
        Event ev;
        c->uni_pending = false;
        c->b2.keep.pending = c->b2.surv_known = false;
        rc = colibri_train_once(c, o, &ev);
        // the class counts this attempt left are the next run's only if it ended well: an attempt that failed, overflowed or is repeated counts again
        c->uni_cached  = rc == COLIBRI_OK && (c->uni_cached || c->uni_pending);
        c->uni_pending = false;
        // ... and order 2's partition likewise, and only from a run that needed no repeat and saw no overflow flag: a repeated run leaves nothing behind
        c->b2.keep.valid = rc == COLIBRI_OK && ladder.retries == 0 && !c->hstate.overflow && !c->hstate.radix_overflow && (c->b2.keep.valid || c->b2.keep.pending);
        c->b2.keep.pending = c->b2.surv_known = false;
        dump_kernel_clocks();
        const bool small_passes_apply = retry_with_small_passes(c->npos);  // (as the attempt saw it: before its flags are cleared)
        c->b2.disabled = c->b2.chain_disabled = tl_small_passes = false;
        Step st;
        if (rc == kRetry) {
            st = advance(ladder, c->split_exact, opt_in->table_mode, small_passes_apply, ev);
            if (st.verdict == Verdict::kFail)
                rc = fail(c, COLIBRI_ERR_OVERFLOW, "the radix path overflowed (%s; region %llu records, %u positions; table_mode = 2 forbids the global-table rerun)",
                          ev.overflow == 1 ? "an A-bin region" : ev.overflow == 2 ? "a final bin outgrew its LDS table" : "survivor id range", (unsigned long long)(c->recs[0].n / kASlots),
                          c->npos);
            else if (st.verdict != Verdict::kRepeat)
                rc = fail(c, COLIBRI_ERR_STATE, "colibri_train: an order loop reported an event that asks for no repeat");  // (the loops' guards are the ladder's)
        }
        if (rc != kRetry) {
            // a result buffer ran out (a corpus that keeps unusually many patterns per position: duplicated text): more room, again
            // (one result per position and order — with skipgrams one per gap mask as well: up to ~6 x 10^5 masks for a window of 31 tokens)
            const uint64_t per_window = (opt_in->doskipgrams || opt_in->doskipgrams_exhaustive) ? 700000ull : 1ull;
            const uint64_t bound = (uint64_t)std::max(1, std::min<int>(opt_in->maxlength, COLIBRI_MAX_ORDER - 1)) * ((uint64_t)c->npos + 1) * per_window;
            if (rc != COLIBRI_ERR_OVERFLOW || !c->hstate.overflow || c->res_cap_used >= std::min<uint64_t>(0x7FFFFFF0ull, bound)) break;
            ev      = Event{};
            ev.what = What::kResults;
            st      = advance(ladder, c->split_exact, opt_in->table_mode, small_passes_apply, ev);
        }
        const bool debug = getenv("COLIBRI_DEBUG_OVERFLOW") != nullptr;
        const bool plain = ev.what == What::kOverflow && ev.loop == Loop::kPlain;
        if (debug && plain && st.reason == COLIBRI_FALLBACK_CHAIN) explain_chain_overflow(c);
        if (debug) fprintf(stderr, "colibri: the run is repeated (COLIBRI_FALLBACK_* %d)\n", st.reason);
        if (debug && plain && st.reason == COLIBRI_FALLBACK_ORDER2) explain_order2_overflow(c, small_passes_apply);
        if (st.set_split_exact) c->split_exact = true;  // (for this corpus: reset by the next upload)
        if (st.reason == COLIBRI_FALLBACK_RESULTS) c->res_scale *= 4;
        c->run_fallback = ladder.first_reason;
        c->run_retries  = ladder.retries;
    }
    c->res_scale = 1;
    if (stats_out && rc == COLIBRI_OK) {
        *stats_out                 = c->stats;
        stats_out->path            = c->run_path;
        stats_out->fallback_reason = c->run_fallback;
        stats_out->retries         = c->run_retries;
        stats_out->reserved_       = 0;
    }
    return rc;
}
