/* include/colibri_hip.h — the C ABI of libcolibri_hip.so (MI355X / gfx950).
 *
 * This is the drop-in boundary of the hot path: the reference has no FFI layer of its
 * own, its path sits behind C++ template methods; these entry points are what a binding for that path
 * would call. The C++ face in colibri-core_amd/host/ (PatternModelOptions / PatternModel<uint32_t> /
 * IndexedPatternModel<> / IndexedCorpus with the reference's names and signatures) is implemented on
 * top of exactly these functions. Plain pointers and sizes only; no exceptions, no STL, no torch types.
 *
 * Every function returns COLIBRI_OK (0) or a negative status; colibri_last_error() gives the message the
 * C++ face prints before throwing InternalError (reference include/common.h:41-44). There is no CPU
 * fallback anywhere behind this interface: without a usable HIP device colibri_create fails.
 *
 * One context per host thread (the reference is not thread-safe either, include/classencoder.h:193-207).
 */
#ifndef COLIBRI_HIP_H
#define COLIBRI_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define COLIBRI_ABI_VERSION 4 /* 4: colibri_stats says which engines counted the run and why it was repeated, if it was (path, fallback_reason, retries: round 6). 3: colibri_kshard_emit / _count / _apply carry 4-byte keys, bit + number feedback (round 4). 2: colibri_train leaves stats.keybytes at 0 (colibri_result_sizes computes it), kernel classes 11..14, colibri_kshard_*, colibri_stream */
#define COLIBRI_MAX_ORDER 128 /* per-order statistics are kept for n < 128; MAXLENGTH defaults to 100 in the reference */

enum {
    COLIBRI_OK              = 0,
    COLIBRI_ERR_ARG         = -1,  /* NULL / out-of-range argument                                         */
    COLIBRI_ERR_HIP         = -2,  /* a HIP runtime call failed (message has the call and hipGetErrorString) */
    COLIBRI_ERR_NODEVICE    = -3,  /* no gfx950-class device visible                                       */
    COLIBRI_ERR_UNSUPPORTED = -4,  /* options outside the accelerated subset            */
    COLIBRI_ERR_CORPUS      = -5,  /* corpus not usable: > 4 GiB per device, token > 8 bytes, flexgram class  */
    COLIBRI_ERR_STATE       = -6,  /* call order: no corpus uploaded / not trained yet                     */
    COLIBRI_ERR_OVERFLOW    = -7   /* a device table or result buffer was exhausted                        */
};

typedef struct colibri_ctx colibri_ctx;

/* POD mirror of the PatternModelOptions fields PatternModel::train reads on this path
 * (reference include/patternmodel.h:103-213; defaults :153-180). */
typedef struct colibri_options {
    /* Every combination colibri_train does not run is refused with COLIBRI_ERR_UNSUPPORTED / _ARG and a message (check_options in
     * csrc/colibri_hip.hip is the authority; the comments below follow it). "constraint set" = colibri_set_constraint is in force. */
    int32_t mintokens;              /* MINTOKENS: -1 -> 2, 0 -> 1 (patternmodel.h:883-886); any value >= 1 (1: every window is kept)    */
    int32_t maxlength;              /* MAXLENGTH (default 100), >= 1; per-order statistics are kept below COLIBRI_MAX_ORDER              */
    int32_t minlength;              /* MINLENGTH (default 1): > 1 only with a constraint set (the C++ face drops the short patterns of an
                                       unconstrained run itself, after the run)                                                        */
    int32_t maxbackofflength;       /* MAXBACKOFFLENGTH: >= maxlength (no effect), or 1 <= b < maxlength with mintokens >= 2, without
                                       skipgrams or a constraint set: orders above b + 1 look back at the b-token sub-patterns only     */
    int32_t mintokens_unigrams;     /* MINTOKENS_UNIGRAMS (-W): > mintokens = secondary word threshold; needs mintokens >= 2, no
                                       constraint set, table_mode != 2                                                                 */
    int32_t mintokens_skipgrams;    /* MINTOKENS_SKIPGRAMS (raised to mintokens when lower, :887-888)                                   */
    int32_t minskiptypes;           /* MINSKIPTYPES (default 2): distinct fillers a skipgram of an indexed model needs                  */
    int32_t maxskips;               /* MAXSKIPS (default 3), >= 1                                                                       */
    int32_t doskipgrams;            /* DOSKIPGRAMS: indexed models only (the reference's rule, :1558); not with a constraint set        */
    int32_t doskipgrams_exhaustive; /* DOSKIPGRAMS_EXHAUSTIVE: unindexed models only; not together with doskipgrams (:958-963); not with
                                       a constraint set. Either kind: patterns of more than 13 tokens stop the run when they turn up     */
    int32_t dopatternperline;       /* DOPATTERNPERLINE (-L): every line is one pattern; needs mintokens = 1, minlength = 1, unindexed,
                                       no skipgrams, no constraint set                                                                 */
    int32_t prunenonsubsumed;       /* PRUNENONSUBSUMED: must be 0 here (a post-hoc pass over the finished model: colibri_subsume_resident)  */
    int32_t prunesubsumed;          /* PRUNESUBSUMED: must be 0 here (same)                                                             */
    int32_t indexed;                /* 0: PatternModel<uint32_t> (model type 10), 1: IndexedPatternModel<> (20)                         */
    int32_t profile;                /* 1: bracket every kernel class with HIP events (colibri_kernel_time); 2: only the class that holds the
                                       dominant kernel of the path the run takes (K_COUNT2 / K_BINCOUNT / K_COUNT): 2 events per step   */
    int32_t table_mode;             /* 0: automatic; 1: force the global open-addressed table; 2: force radix-partition + LDS count     */
} colibri_options;

/* What train() reports: the numbers the reference keeps in the model (totaltokens/totaltypes/maxn/minn,
 * patternmodel.h:550-556) and prints per order on stderr (:1195-1245). */
typedef struct colibri_stats {
    uint64_t totaltokens;                  /* sum of sentence lengths (patternmodel.h:1047-1048)            */
    uint64_t totaltypes;                   /* distinct unigrams BEFORE pruning (:1199-1201)                  */
    uint64_t npatterns;                    /* size of the final model                                        */
    uint64_t keybytes;                     /* sum of key byte lengths over the final model: 0 in what colibri_train returns (serialised sizes
                                              are not part of counting); colibri_result_sizes computes and reports it                       */
    uint64_t nrefs;                        /* indexed: total index entries                                   */
    uint64_t nsentences;                   /* sentences incl. empty ones                                     */
    int32_t  maxn, minn;                   /* as PatternModel::maxlength()/minlength()                       */
    uint64_t windows[COLIBRI_MAX_ORDER];   /* W_n: n-token windows inside sentences (line.ngrams(), :1063)    */
    uint64_t admitted[COLIBRI_MAX_ORDER];  /* P_n: windows that passed the look-back and were counted        */
    uint64_t found[COLIBRI_MAX_ORDER];     /* distinct new patterns of order n before pruning                */
    uint64_t pruned[COLIBRI_MAX_ORDER];    /* erased by prune()/pruneskipgrams() at order n                  */
    uint64_t kept[COLIBRI_MAX_ORDER];      /* found - pruned                                                 */
    double   train_ms;                     /* wall time of the device work of train(), host clock            */
    /* ABI 4: which engines counted the run (COLIBRI_PATH_* bits, of the LAST attempt — the one whose model this is), and whether the run was repeated: an order that does
     * not fit the engine it started on (a record region, a final bin's LDS table, the key bits) ends the attempt, and the whole run is done again, exactly, on the
     * next engine down — a 2-10 x cost a caller could only see with COLIBRI_DEBUG_OVERFLOW before. fallback_reason: COLIBRI_FALLBACK_* of the FIRST repeat (0: none);
     * retries: repeats in all (the result buffers growing counts as one). */
    int32_t  path, fallback_reason, retries, reserved_;
} colibri_stats;
enum {
    COLIBRI_PATH_TABLE   = 1,  /* the global open-addressed table (device atomics): table_mode = 1, or the last resort                                   */
    COLIBRI_PATH_RADIX   = 2,  /* the radix path: records partitioned twice, counted in LDS (first-generation kernels for the orders the bits below do not name) */
    COLIBRI_PATH_BI2     = 4,  /* ... order 2 on the second-generation engine (8-byte records, dense head, one wave per final bin)                        */
    COLIBRI_PATH_CHAIN   = 8,  /* ... orders >= 3 on that engine too (keys = (number of the leading (n-1)-gram, class))                                    */
    COLIBRI_PATH_WIDE    = 16, /* ... in its form for 2.15 - 4.3 x 10^8 positions (eight sub-regions, 2048-slot tables)                                     */
    COLIBRI_PATH_SLICED  = 32, /* an order counted in several passes over slices of its keys (corpora beyond one pass)                                      */
    COLIBRI_PATH_PER_PASS = 64, /* the id-keeping kinds' loop: one host look-up per pass (indexed / skipgram models off the enqueued loop, constrained runs)  */
    /* how an indexed model's references (sentence, token) travelled to the forward index's sort; neither bit: as two 32-bit arrays (id | sentence, token) */
    COLIBRI_PATH_PAIRS_WHOLE    = 128, /* ... as whole packed 64-bit pairs (id, sentence, token in one word): 33 bits of sentence and token, or a sentence of >= 65536 tokens */
    COLIBRI_PATH_PAIRS_UNPACKED = 256  /* ... as id << 32 | position, looked up after the sort: sentence and token need more than 33 bits                 */
};
enum {
    COLIBRI_FALLBACK_NONE      = 0,
    COLIBRI_FALLBACK_REGION    = 1,  /* an A-bin region of the first-generation radix path outgrew its room   -> global table                */
    COLIBRI_FALLBACK_BIN       = 2,  /* a final bin outgrew its LDS table (hash skew)                          -> global table                */
    COLIBRI_FALLBACK_IDS       = 3,  /* survivor id range exhausted                                            -> global table                */
    COLIBRI_FALLBACK_ORDER2    = 4,  /* the second-generation order 2 could not hold the corpus               -> smaller passes, or first-generation kernels */
    COLIBRI_FALLBACK_SPLIT     = 8,  /* a run of a sliced order's direct split outgrew its room                -> the exact split             */
    COLIBRI_FALLBACK_CHAIN     = 16, /* an order >= 3 did not fit the chained engine (key bits, region, bin)   -> first-generation orders >= 3 */
    COLIBRI_FALLBACK_RESULTS   = 32, /* the result buffers were too small (duplicated text)                    -> four times the room         */
    COLIBRI_FALLBACK_PAIRS     = 64, /* an index with more references than the pair buffer started with       -> a larger buffer             */
    COLIBRI_FALLBACK_LDS_ORDER = 128 /* a checked rank of the forward index's build disagreed (ranks from LDS adds) -> every rank matched with ballots */
};

/* kernel classes for colibri_kernel_time */
enum {
    COLIBRI_K_TOKENISE = 0, /* byte stream -> token-start vector (upload time, not train)        */
    COLIBRI_K_CLEAR    = 1, /* table reset                                                       */
    COLIBRI_K_COUNT    = 2, /* scan + SpookyHash + hash-table build: the dominant kernel         */
    COLIBRI_K_PRUNE    = 3, /* threshold prune + survivor compaction                             */
    COLIBRI_K_RESOLVE  = 4, /* per-position survivor ids for the next order                      */
    COLIBRI_K_SKIPGRAM = 5, /* skipgram counting                                                 */
    COLIBRI_K_INDEX    = 6, /* forward-index build                                               */
    COLIBRI_K_EXPORT   = 7,
    COLIBRI_K_EMIT     = 8,  /* binned path: scan + SpookyHash + block-local reduce -> (key, position, count) records */
    COLIBRI_K_SCATTER  = 9,  /* binned path: two-level radix partition of the records by hash bits            */
    COLIBRI_K_BINCOUNT = 10, /* binned path: per-bin LDS hash build + threshold + survivor ids                */
    COLIBRI_K_EMIT2    = 11, /* order 2, second generation: scan -> dense head histogram | 8-byte records by A bin */
    COLIBRI_K_LEVELB2  = 12, /* ... one block partitions one (sub-region, A bin) slot by B bin                  */
    COLIBRI_K_COUNT2   = 13, /* ... one wave per final bin: LDS table, threshold, survivors, positions          */
    COLIBRI_K_LISTS2   = 14, /* ... survivor positions -> bucket lists -> bitmap -> active list of order 3      */
    COLIBRI_K_JOIN     = 15, /* seeded run: the order's distinct keys against the seed set (and the look-back's seed ids) */
    COLIBRI_K_NCLASSES = 16
};

/* ---- lifecycle ------------------------------------------------------------------------------- */
int         colibri_abi_version(void);
int         colibri_create(colibri_ctx** out, int device); /* device = HIP ordinal                  */
void        colibri_destroy(colibri_ctx* ctx);
const char* colibri_last_error(const colibri_ctx* ctx);   /* never NULL                            */

/* ---- corpus: replaces IndexedCorpus::load (reference src/pattern.cpp:1916-1967) ------------------
 * payload = the .colibri.dat v2 file minus its 2-byte header (A2 02). first_sentence = the index given
 * to the first sentence (train()'s `firstsentence`, patternmodel.h:880-881,896; 1 by default) — this is
 * also how a sentence-sharded rank keeps global sentence numbers. The bytes are copied to HBM and
 * tokenised there (token-start vector + sentence table). */
int colibri_upload_corpus(colibri_ctx* ctx, const uint8_t* payload, uint64_t nbytes, uint32_t first_sentence);
/* same, for bytes that already live in this device's HBM (no PCIe copy; a device-to-device copy is made) */
int colibri_upload_corpus_device(colibri_ctx* ctx, const void* device_payload, uint64_t nbytes, uint32_t first_sentence);
/* tokens (delimiters excluded), sentences (empty ones included), highest class id */
int colibri_corpus_info(const colibri_ctx* ctx, uint64_t* ntokens, uint64_t* nsentences, uint64_t* maxclass);

/* ---- training: replaces PatternModel::train (reference include/patternmodel.h:880-1345) and, for
 * indexed models, IndexedPatternModel::train/trainskipgrams (:2828-2844, :2969-3010). All orders run on
 * the device without a host round trip per order. */
int colibri_train(colibri_ctx* ctx, const colibri_options* opt, colibri_stats* stats);

/* ---- results: replaces iteration over PatternMap + valuehandler.write (patternstore.h:534-542,
 * datatypes.h:219-221,263-270). Caller allocates from colibri_result_sizes():
 *   key_off[npatterns+1], key_bytes[keybytes], counts[npatterns]
 *   indexed: ref_off[npatterns+1], ref_sentence[nrefs], ref_token[nrefs]; refs sorted by (sentence, token).
 * Keys are the pattern's bytes without the trailing 00 (a skipgram's gaps are the byte 03). Order: by
 * pattern length n, unspecified inside an order (the reference's order is unordered_map order). */
int colibri_result_sizes(colibri_ctx* ctx, uint64_t* npatterns, uint64_t* keybytes, uint64_t* nrefs); /* the first call after a train computes the key lengths on the device */
int colibri_export_unindexed(colibri_ctx* ctx, uint64_t* key_off, uint8_t* key_bytes, uint32_t* counts);
int colibri_export_indexed(colibri_ctx* ctx, uint64_t* key_off, uint8_t* key_bytes, uint32_t* counts, uint64_t* ref_off,
                           uint32_t* ref_sentence, uint16_t* ref_token);

/* ---- sentence-sharded multi-GPU training (one context per rank; the collectives themselves are the caller's: RCCL through
 * torch.distributed in colibri_amd.dist, or any all-to-all). The reference has no counterpart — it is single-threaded; these
 * entry points split PatternModel::train's order loop (patternmodel.h:981-1270) and the skipgram passes (:1163-1171, :2969-3010)
 * at their only cross-shard dependency: the global count of a candidate pattern. Survivor ids are GLOBAL (handed out by the owner
 * rank of a key), so the 64-bit keys of all ranks are comparable and counts are summed exactly. All *_dev arguments are DEVICE
 * pointers. A "pass" is identified by (n, mask, level): mask 0 = the n-gram pass of order n; mask != 0 = level 1..parts-1 of the
 * skipgram (n, mask), whose identity is built by pairing the global ids of its contiguous parts left to right.
 *   per pass:  shard_count -> [all-to-all sizes] -> shard_send -> [all-to-all keys, counts (, aux)] -> shard_merge ->
 *              [all-gather found, kept] -> shard_reply -> [all-to-all replies back] -> shard_apply ;  at the end: shard_finish.
 * Each rank then exports (colibri_export_unindexed + colibri_shard_export_gids) the patterns it was named exporter of — the
 * union over ranks is the model — and, for indexed models, its LOCAL forward index keyed by global id
 * (colibri_shard_export_index); a pattern's index is the concatenation of the ranks' runs in rank order (sentence ranges of
 * the ranks are disjoint and ascending, so that concatenation is already sorted). */
int colibri_shard_begin(colibri_ctx* ctx, const colibri_options* opt, int world);
/* local count of pass (n, mask, level), then this rank's distinct candidates partitioned by owner = hash(key) % world */
int colibri_shard_count(colibri_ctx* ctx, int n, uint32_t mask, int level, uint64_t* ncandidates, uint64_t* per_owner /* [world] */);
/* copy the partitioned candidates into the caller's send buffers: keys u64[ncandidates], counts u32[ncandidates],
 * aux u32[ncandidates] (distinct-source counts of indexed skipgrams; zeros otherwise; may be NULL when not wanted) */
int colibri_shard_send(colibri_ctx* ctx, void* keys_dev, void* counts_dev, void* aux_dev);
/* the same without a copy: the library's own partitioned buffers (device pointers, valid until the next colibri_shard_count; *aux_dev = NULL when the pass has none) */
int colibri_shard_send_view(colibri_ctx* ctx, void** keys_dev, void** counts_dev, void** aux_dev);
/* owner side: merge the records received from every rank (concatenated in rank order; per_src[r] records from rank r) */
int colibri_shard_merge(colibri_ctx* ctx, const void* keys_dev, const void* counts_dev, const void* aux_dev, const uint64_t* per_src /* [world] */,
                        uint64_t* found, uint64_t* kept);
/* owner side: assign global survivor ids gid_base.. to the kept keys and fill one reply per received record
 * (reply_gid: u32 global id | bit 31 = "you export it", 0xFFFFFFFF = pruned; reply_cnt: u32 global count) */
int colibri_shard_reply(colibri_ctx* ctx, uint32_t gid_base, void* reply_gid_dev, void* reply_cnt_dev);
/* contributor side: apply the replies (same order as the records sent) and write global survivor ids per position */
int colibri_shard_apply(colibri_ctx* ctx, const void* reply_gid_dev, const void* reply_cnt_dev, uint64_t* exported, uint64_t* admitted);
/* order 1 on class-indexed arrays (the north star's "all-reduce of the per-bucket count tables before the prune"): when every rank's
 * encoding is canonical (eligible) the unigram pass needs no key exchange — each rank fills cnt[nclasses] (u32 per class id) and
 * minrank[nclasses] (its rank where it saw the class, else 0x7FFFFFFF), the caller all-reduces them (SUM / MIN), and every rank
 * applies the reduced arrays. The global id of a unigram is its class id; later passes must start their ids at nclasses. */
int colibri_shard_uni_info(const colibri_ctx* ctx, int* eligible, uint64_t* maxclass);
int colibri_shard_uni_count(colibri_ctx* ctx, void* cnt_dev, void* minrank_dev, uint32_t nclasses, int rank);
int colibri_shard_uni_apply(colibri_ctx* ctx, const void* cnt_global_dev, const void* minrank_global_dev, uint32_t nclasses, int rank, uint64_t* found, uint64_t* kept,
                            uint64_t* exported);
/* close the run: global per-order found / kept (caller-reduced), global token count; fills stats like colibri_train */
int colibri_shard_finish(colibri_ctx* ctx, const uint64_t* found_global, const uint64_t* kept_global, uint64_t totaltokens_global, int maxn, colibri_stats* stats);
/* global id of every pattern this rank exports, in the order of colibri_export_unindexed (gids[npatterns]) */
int colibri_shard_export_gids(colibri_ctx* ctx, uint32_t* gids);
/* indexed models: this rank's forward index — gids[ngids] ascending, ref_off[ngids+1], sentence/token[nrefs] */
int colibri_shard_index_sizes(const colibri_ctx* ctx, uint64_t* ngids, uint64_t* nrefs);
int colibri_shard_export_index(colibri_ctx* ctx, uint32_t* gids, uint64_t* ref_off, uint32_t* ref_sentence, uint16_t* ref_token);

/* ---- key-sharded multi-GPU training of the plain n-gram model (BASELINE.json configs[2]; csrc/kshard.hpp). The reference has no counterpart (it is
 * single-threaded); what is distributed is PatternModel::train's order loop (include/patternmodel.h:981-1270) at its only cross-shard dependency, the GLOBAL count
 * of a candidate before the prune of its order (:1195-1245). Unlike colibri_shard_* above, no rank counts candidates it does not own: every rank scans its own
 * sentences into RECORDS (the single-device emit kernels), the records travel to the owner of their key (owner = top bits of the key's mix), the owner counts them
 * with the single-device kernels and applies the threshold to the exact global count, and only what survived travels back (order 2: positions of surviving windows;
 * order >= 3: global survivor ids of surviving records; plus one (representative, count) per kept pattern to the rank that exports it). Order 1 is an all-reduce
 * (SUM) of the dense per-class count array — the north star's "all-reduce of the per-bucket count tables before the prune". world = 1, 2, 4 or 8.
 * The collectives are the caller's (host/src/sharded.cpp: RCCL, or device copies); all device work is enqueued on colibri_stream(ctx), which the caller hands to
 * its collectives too: an order costs two host look-ups (the sizes of the two exchanges). All *_dev arguments are DEVICE pointers owned by the library.
 *   colibri_kshard_info on every rank -> [the caller checks that all ranks are eligible, takes the maxima] -> colibri_kshard_begin
 *   order 1:    colibri_kshard_uni_count -> [all-reduce SUM, u32 x nclasses, in place] -> colibri_kshard_uni_apply
 *   order n>=2: colibri_kshard_emit -> [sizes] -> colibri_kshard_recv_buffers -> [all-to-all records, tables; order 2: all-reduce head rows SUM / MIN] ->
 *               colibri_kshard_count -> [sizes] -> colibri_kshard_feedback_buffers -> [all-to-all feedback, exports] -> colibri_kshard_apply
 *               (the loop ends after the order at which no rank admitted a window: the reference's "None found", :1189-1194)
 *   end:        colibri_kshard_local_stats -> [sums over ranks] -> colibri_kshard_finish; then colibri_result_sizes / colibri_export_unindexed on every rank:
 *               each pattern of the model is exported by exactly one rank (the lowest that holds an occurrence; rank 0 for unigrams). */
void* colibri_stream(colibri_ctx* ctx); /* the hipStream_t all of the context's device work is enqueued on */
int colibri_kshard_info(colibri_ctx* ctx, const colibri_options* opt, int* eligible, uint64_t* maxclass, uint64_t* npositions);
int colibri_kshard_begin(colibri_ctx* ctx, const colibri_options* opt, int world, int rank, uint64_t maxclass_global, uint64_t maxpositions_global);
int colibri_kshard_uni_count(colibri_ctx* ctx, void** cnt_dev, uint32_t* nclasses);
int colibri_kshard_uni_apply(colibri_ctx* ctx);
/* est_records: an upper bound of the order's records over ALL ranks (order 2: the corpus' tokens; above: the windows that survived the order below), ids_global: the
 * numbers the order below handed out over all ranks (colibri_kshard_apply's *ids_global) — the same values on every rank; more: order n + 1 follows.
 * per_owner[world]: keys for each rank, in rank order in *send_dev (*recbytes = 4 each: the source has partitioned its records completely, a key is what the final bin
 * does not fix); *tab_dev: u32[world][*tab_words] (the runs' lengths per (owner, bin)), row d goes to rank d;
 * *head_dev: order 2: u32[2][4096] (row 0: all-reduce SUM, row 1: all-reduce MIN, in place), else NULL; *admitted: windows this rank counted at order n */
int colibri_kshard_emit(colibri_ctx* ctx, int n, uint64_t est_records, uint64_t ids_global, int more, void** send_dev, void** tab_dev, uint32_t* tab_words, uint64_t* per_owner,
                        uint32_t* recbytes, void** head_dev, uint64_t* admitted);
int colibri_kshard_recv_buffers(colibri_ctx* ctx, uint64_t nrecords, void** recv_dev /* keys, concatenated in source order */, void** tab_recv_dev /* u32[world][tab_words], row s from rank s */);
/* per_src[world]: keys received from each rank. more: order n + 1 follows (feedback is produced). fb_per_dst [world]: feedback for each rank, in rank order in *fb_dev, in
 * units of *fb_bytes (= 4): per source, in the order it sent, one bit per key, then the dense number of every surviving key's window; ex_per_dst: exports (8 bytes each) in
 * *ex_dev; *kept_bins: the keys this owner kept (the caller gathers them over the ranks: colibri_kshard_apply's kept_per_owner) */
int colibri_kshard_count(colibri_ctx* ctx, int n, const uint64_t* per_src, int more, void** fb_dev, uint64_t* fb_per_dst, uint32_t* fb_bytes, void** ex_dev, uint64_t* ex_per_dst,
                         uint64_t* kept_bins);
/* after colibri_kshard_count of order 2: the windows of the surviving head pairs (both classes < 64: counted densely, on no owner's list) over ALL ranks — the same value
 * on every rank (the head counts are all-reduced); with the feedback sizes it bounds order 3's records exactly. No device look-up: read with the count step's sizes. */
int colibri_kshard_head_windows(const colibri_ctx* ctx, uint64_t* windows);
int colibri_kshard_feedback_buffers(colibri_ctx* ctx, uint64_t nfeedback, uint64_t nexports, void** fb_recv_dev, void** ex_recv_dev); /* each concatenated in owner order */
/* fb_src / ex_src [world]: feedback units / exports received from each owner; kept_per_owner[world]; *ids_global: the numbers order n handed out over all ranks */
int colibri_kshard_apply(colibri_ctx* ctx, int n, const uint64_t* fb_src, const uint64_t* ex_src, const uint64_t* kept_per_owner, int more, uint64_t* ids_global);
/* arrays of COLIBRI_MAX_ORDER: distinct keys / survivors among the keys this rank OWNS (order 1: global, on rank 0 only), windows it counted; *syncs: host look-ups so far */
int colibri_kshard_local_stats(colibri_ctx* ctx, uint64_t* found, uint64_t* kept, uint64_t* admitted, uint32_t* syncs);
int colibri_kshard_finish(colibri_ctx* ctx, const uint64_t* found_global, const uint64_t* kept_global, const uint64_t* admitted_global, uint64_t totaltokens_global, int maxn,
                          colibri_stats* stats);

/* ---- parity / measurement hooks ------------------------------------------------------------------ */
/* SpookyHash::Hash64 (reference include/SpookyV2.h:59-66) of every n-token window, computed by the same
 * device routine the count kernel uses: out[i] for token position i (delimiters are positions too);
 * 0 where no n-token window starts. out has colibri_positions() entries. */
int colibri_hash_windows(colibri_ctx* ctx, int n, uint64_t* out_host);
int colibri_positions(const colibri_ctx* ctx, uint64_t* npositions);
/* Which implementation of the counting stage the last colibri_train ran (the reference has one, include/patternmodel.h:1078-1178; here the choice follows
 * the corpus and colibri_options.table_mode, and an overflow of the radix path repeats the run on the table): 1 = global open-addressed table,
 * 2 = radix partition + LDS count, 0 = neither (pattern list, or nothing trained). *passes (optional) = passes over key slices the order-2 stage used. */
int colibri_last_mode(const colibri_ctx* ctx, int* passes);
/* What the dominant kernel of the last plain run processed at order 2 (second-generation kernels, colibri_last_mode = 2): *records = the 8-byte records
 * bi2_count_kernel read (in a key-sharded run: the records this rank counted as an owner); *head_windows = the admitted bigram windows whose two classes are both
 * < 64 — counted in the scan's dense LDS histogram, never records (0 in a key-sharded run). bench.py prices the kernel by these. */
int colibri_order2_records(colibri_ctx* ctx, uint64_t* records, uint64_t* head_windows);
/* SpookyHash::Hash64 of nkeys independent byte strings (off[nkeys+1] into bytes) on the device */
int colibri_hash_keys(colibri_ctx* ctx, const uint8_t* bytes, const uint64_t* off, uint64_t nkeys, uint64_t* out_host);
/* accumulated HIP-event time and launch count of one kernel class since the last colibri_train() began
 * (only when options.profile = 1; events are recorded on the library's own stream) */
int colibri_kernel_time(const colibri_ctx* ctx, int kernel_class, double* total_ms, uint64_t* launches);

/* ---- constrained training -------------------------------------------------------------------------------------------
 * Replaces PatternModel::train(..., constrainbymodel) (reference include/patternmodel.h:1062-1072, :1088-1089, :1209-1217): while a
 * constraint set is installed, colibri_train counts — in one pass per length MINLENGTH..MAXLENGTH, without look-back — exactly the
 * windows whose key bytes are a member, and keeps those that reach MINTOKENS (any value >= 1). key_off[npatterns + 1] / key_bytes: the
 * patterns' keys as in colibri_export_unindexed (skipgram / flexgram keys never equal a window and are simply never hit).
 * npatterns = 0 removes the constraint. stats.totaltypes is 0 after a constrained run (the reference leaves it unset there). */
int colibri_set_constraint(colibri_ctx* ctx, const uint64_t* key_off, const uint8_t* key_bytes, uint64_t npatterns);
/* Continued training: replaces PatternModel::train(..., continued = true) on a model that already holds patterns (reference
 * include/patternmodel.h:983-995 "Skipping n-grams, already in model", colibri-patternmodeller -E). The patterns of that model are installed
 * like a constraint set; the next colibri_train then counts only the orders the model has no n-grams of, and the look-back of those orders
 * (:1139-1152) finds the loaded patterns as well as the new survivors. The results are the NEW patterns only (the caller already has the
 * others); stats.totaltokens is the corpus' (the reference leaves the model's total untouched: the C++ face ignores it). MINTOKENS >= 2,
 * no skipgrams. npatterns = 0 (or colibri_set_constraint) ends the mode. */
int colibri_set_continuation(colibri_ctx* ctx, const uint64_t* key_off, const uint8_t* key_bytes, uint64_t npatterns);
/* Filtered training: replaces PatternModel::train(..., filter) (reference include/patternmodel.h:899-914, :1106-1137). While a filter set is installed, colibri_train
 * counts at every order exactly the windows that contain one of the set's n-grams (as a sub-n-gram of any length) or are an instance of one of its skipgrams
 * (same length, non-gap tokens equal; flexgrams match nothing, src/pattern.cpp:1760-1785) — without look-back, then prunes by MINTOKENS per order; the run ends at
 * the first order that finds nothing (MINTOKENS = 1: after MAXLENGTH). MINLENGTH = 1, no skipgrams. npatterns = 0 (or colibri_set_constraint) ends the mode. */
int colibri_set_filter(colibri_ctx* ctx, const uint64_t* key_off, const uint8_t* key_bytes, uint64_t npatterns);
/* Expanding a loaded model on further corpus data: replaces PatternModel::train(..., continued = false) on a model that already holds patterns (reference
 * include/patternmodel.h:880-1270, colibri-patternmodeller -i model -f corpus -e N without -E). The model's n-grams are installed as a SEED set: the keys as for
 * colibri_set_constraint (distinct; a skipgram or flexgram key is refused with COLIBRI_ERR_UNSUPPORTED) and counts[p], the pattern's count in the loaded model
 * (an indexed model's: its number of references). The next colibri_train then, for every order n = 1 .. MAXLENGTH: counts the windows of the corpus whose two
 * (n-1)-token sub-windows are keys of the model as it stands (loaded or new, after that order's prune); joins the order's distinct keys with the seed set —
 * stats.found[n] is the number of keys the order CREATED, those no seed has —; stops BEFORE the prune when it created none (that order's rows are all seeds,
 * exported unpruned with their summed counts; no higher order is visited); otherwise prunes every key of n tokens, loaded ones included, whose loaded + new
 * count is below MINTOKENS. The results are the surviving patterns that occur in the corpus, with SUMMED counts (an indexed run: the corpus' references only);
 * colibri_seed_fetch tells what became of the seeds. stats.kept[n] = the order's result rows, created or loaded; stats.pruned[n] = what prune(MINTOKENS, n) erased: the
 * order's distinct keys that were not kept plus the loaded patterns of n tokens that never occurred and lie below MINTOKENS (0 at the order the run stopped at and at
 * orders it never visited). A loaded count plus the corpus' must fit 32 bits (COLIBRI_ERR_OVERFLOW otherwise). stats.maxn is the last order that created a key: the run stopped at maxn + 1 if that is <= MAXLENGTH.
 * stats.totaltypes = npatterns + found[1], the reference's size() at order 1 (0 when the run stopped there); stats.totaltokens is the corpus'.
 * MINTOKENS >= 2, MINLENGTH = 1, no skipgrams, back-off length, word threshold or pattern list; one device; npatterns < 2^31 - 16. The run is counted on the
 * global table (stats.path = TABLE | PER_PASS). npatterns = 0 (or any other colibri_set_* call) ends the mode. */
int colibri_set_seed(colibri_ctx* ctx, const uint64_t* key_off, const uint8_t* key_bytes, const uint32_t* counts, uint64_t npatterns);
/* After a seeded colibri_train, for every seed pattern p (npatterns entries each): row_of_seed[p] = the result row (colibri_export_*) that carries it, or
 * 0xFFFFFFFF when none does; kept[p] = 1 when it stays in the model. At an order the run pruned a seed stays iff its row was kept, or it does not occur in the
 * corpus and counts[p] >= MINTOKENS; at the order the run stopped at and above, every seed stays. */
int colibri_seed_fetch(colibri_ctx* ctx, uint32_t* row_of_seed, uint8_t* kept);

/* ---- class encoder: plain text -> word frequency list -> class-encoded corpus -------------------------------------
 * Replaces the corpus-proportional work of ClassEncoder::processcorpus (reference src/classencoder.cpp:156-188: the word frequency
 * list) and ClassEncoder::encodefile / encodestring (:369-436, :550-600: words -> varint classes, one 00 per line). The class of
 * every DISTINCT word is decided by the caller between colibri_text_words and colibri_text_encode (buildclasses :213-229, the
 * unknown-word policy of encodestring :412-424) — that step is proportional to the vocabulary, not to the corpus.
 * Word rules, `rules` = 0 (frequency list) / 1 (encoder): see colibri-core_amd/csrc/textenc.hpp. */
int colibri_text_upload(colibri_ctx* ctx, const uint8_t* text, uint64_t nbytes);                 /* plain text, '\n' ends a line; < 2 GiB */
int colibri_text_count(colibri_ctx* ctx, int rules, uint64_t* nwords, uint64_t* ndistinct);      /* counts every word under `rules`; a call that fails leaves no count behind (words / encode: COLIBRI_ERR_STATE) */
/* one entry per distinct word, in no particular order: byte offset of its FIRST occurrence in the text, its byte length, its count.
 * (The reference fills its unordered_map in first-occurrence order; sorting by first_start reproduces that insertion order.) */
int colibri_text_words(colibri_ctx* ctx, uint32_t* first_start, uint32_t* length, uint32_t* count);
/* cls[k], repeat[k] for distinct word k of the last colibri_text_count(rules = 1): the word becomes `repeat` copies of varint(cls)
 * (0 drops it; "{*3*}" is 3 x class 3). Every '\n' becomes one 00; text after the last '\n' is not encoded (encodefile :569-570).
 * The result is a .colibri.dat v2 payload (no A2 02 header) kept on the device. */
int colibri_text_encode(colibri_ctx* ctx, const uint32_t* cls, const uint32_t* repeat, uint64_t* outbytes, uint64_t* ntokens, uint64_t* nlines);
int colibri_text_fetch(colibri_ctx* ctx, uint8_t* out);                                          /* the encoded payload -> host */
int colibri_text_as_corpus(colibri_ctx* ctx, uint32_t first_sentence);                           /* ... or straight into colibri_upload_corpus_device */

/* ---- flexgrams abstracted from skipgrams ---------------------------------------------------------
 * Replaces IndexedPatternModel::computeflexgrams_fromskipgrams (reference include/patternmodel.h:3724-3744) with
 * Pattern::toflexgram (src/pattern.cpp:145-180) and Pattern::category (:107-127): every SKIPGRAM among the given patterns hands
 * all its references to the flexgram whose key is the skipgram's with each run of {*} (03) tokens replaced by one {**} (04).
 * Input = an indexed model in the layout colibri_export_indexed writes (patterns of other categories are ignored; no corpus is
 * needed). Result, kept on the device until the next call: one entry per distinct flexgram, count = number of references,
 * references ascending by (sentence, token) with duplicates kept (IndexedData::insert is a push_back, datatypes.h:117-119; the
 * reference's own order is its unordered_map's iteration order, and its loop inserts into the map it iterates — the specification
 * here is the loop without that hazard). Grouping is exact (64-bit hash of the collapsed bytes, bytes verified, reseeded on a
 * collision). colibri_flexgrams_fetch copies the result into caller-allocated buffers sized from the three totals
 * (key_off / ref_off: nflexgrams + 1 entries). */
int colibri_flexgrams(colibri_ctx* ctx, const uint64_t* key_off, const uint8_t* key_bytes, const uint64_t* ref_off, const uint32_t* ref_sentence, const uint16_t* ref_token,
                      uint64_t npatterns, uint64_t* nflexgrams, uint64_t* keybytes, uint64_t* nrefs);
/* The same on the indexed model of the last colibri_train of this context, which is still resident in HBM (keys, counts and the forward
 * index never leave the device; only the flexgrams come back through colibri_flexgrams_fetch). COLIBRI_ERR_STATE unless the context holds
 * a trained indexed model of a non-sharded run. */
int colibri_flexgrams_resident(colibri_ctx* ctx, uint64_t* nflexgrams, uint64_t* keybytes, uint64_t* nrefs);
int colibri_flexgrams_fetch(colibri_ctx* ctx, uint64_t* key_off, uint8_t* key_bytes, uint32_t* counts, uint64_t* ref_off, uint32_t* ref_sentence, uint16_t* ref_token);

/* ---- sentence co-occurrence of an indexed model (colibri-patternmodeller -C / -Y) ---------------------------------------------------
 * Replaces IndexedPatternModel::computecooc / computenpmi (reference include/patternmodel.h:3700-3719, :3671-3691): getcooc (:3542-3576) summed over
 * every pattern A of the model. For each reference (s, t) of A in A's own forward index and each occurrence (t2, B) of a pattern of the model the
 * reverse index finds in sentence s (getreverseindex :1746-1824: every window of MINLENGTH..MAXLENGTH tokens of the corpus the model has, and
 * for n >= 3 that window under each gap mask of the model's skipgrams of length n), the pair counts when t2 + n(B) < t or t2 > t + n(A) —
 * adjacent occurrences do not, B == A does. The corpus uploaded to this context (colibri_upload_corpus) is the reverse index.
 *   mode COLIBRI_COOC_COUNT (-C t): B must have a count >= t and the joint count must be >= t (t = 0: every pair; computecooc keeps value >= t).
 *   mode COLIBRI_COOC_NPMI  (-Y x): threshold 0, value = log(joint / (c(A) * c(B))) / -log(joint / total) (:3582-3587; c() is a size_t, total
 *                                   = totaloccurrencesingroup(0, 0), the unsigned sum of the counts), kept when >= x.
 * Rows are ordered by value descending, then A's key bytes, then B's key bytes, ascending (the reference's own tie order is its std::map's of
 * data addresses, and its outputcooc reads freed memory: DESIGN.md §6). Input = an indexed model in the layout colibri_export_indexed writes;
 * a flexgram in it is refused (COLIBRI_ERR_UNSUPPORTED). The result stays on the device until the next call; *nrows rows. Pair events are
 * counted per A occurrence first and processed in chunks of a fixed scratch budget, cut anywhere along the forward index; the partial counts of a
 * pattern cut by a chunk boundary are merged before any threshold (environment: COLIBRI_COOC_CHUNK = events per chunk). */
enum { COLIBRI_COOC_COUNT = 0, COLIBRI_COOC_NPMI = 1 };
int colibri_cooc(colibri_ctx* ctx, const uint64_t* key_off, const uint8_t* key_bytes, const uint64_t* ref_off, const uint32_t* ref_sentence, const uint16_t* ref_token,
                 uint64_t npatterns, uint32_t threshold, int mode, double npmi_threshold, uint64_t* nrows);
/* The same on the indexed model of the last colibri_train of this context, still resident in HBM (pattern numbers = colibri_export_indexed's).
 * COLIBRI_ERR_STATE unless the context holds a trained indexed model of a non-sharded run. */
int colibri_cooc_resident(colibri_ctx* ctx, uint32_t threshold, int mode, double npmi_threshold, uint64_t* nrows);
/* the rows, into caller-allocated arrays of nrows entries (any may be NULL): pattern numbers of A and B, joint count, value (count or NPMI) */
int colibri_cooc_fetch(colibri_ctx* ctx, uint32_t* pattern_a, uint32_t* pattern_b, uint32_t* counts, double* values);
/* what the last call did: pair events, chunks, the peak of the scratch the call takes itself (not counted: the context's radix-sort buffers,
 * the uploaded copy of a loaded model, the result arrays) */
int colibri_cooc_info(const colibri_ctx* ctx, uint64_t* events, uint64_t* chunks, uint64_t* scratch_bytes);

/* ---- pattern relations of an indexed model (colibri-patternmodeller --subsumes / --subsumed / --leftneighbours / --rightneighbours) ------------
 * Replaces the reference's per-pattern loops IndexedPatternModel::getsubchildren / getsubparents / getleftneighbours / getrightneighbours
 * (include/patternmodel.h:3166-3352) run over every pattern A of the model, with category 0, size 0 and no cutoff. For each reference (s, t)
 * of A in A's own forward index and each occurrence (i, B) of a pattern of the model the reverse index finds in sentence s (getreverseindex
 * :1746-1824, as for colibri_cooc), the occurrence counts for
 *   COLIBRI_REL_SUBCHILDREN      t <= i < t + n(A), n(B) <= n(A) - (i - t), B != A
 *   COLIBRI_REL_SUBPARENTS       i <= t, n(B) >= n(A) + (t - i), B != A
 *   COLIBRI_REL_LEFTNEIGHBOURS   i + n(B) == t     (B == A counts)
 *   COLIBRI_REL_RIGHTNEIGHBOURS  i == t + n(A)     (B == A counts)
 *   COLIBRI_REL_INSTANCES        i == t, n(B) == n(A), B an n-gram, B != A      (getinstances :3127-3157; an n-gram A has no rows)
 *   COLIBRI_REL_TEMPLATES        i == t, n(B) == n(A) >= 3, B a skipgram, unless the masked window equals A   (gettemplates :3086-3118)
 * When A or B is a skipgram the two subsumption kinds apply the reference's own tests, which differ from what its comments say: getsubchildren
 * slices A at the corpus token index i, not at i - t, and asks B.instanceof(slice); getsubparents asks A.instanceof(B) of the whole patterns,
 * which only an n-gram A passes, against a skipgram B of its own length at t. B != A is PatternPointer's equality, under which a skipgram whose
 * gap holds a multi-byte token differs from itself. csrc/relations.hpp has the details. The CLI's labels are swapped against the functions
 * (:3622-3662): --rightneighbours prints getleftneighbours as RIGHT-NEIGHBOUR-OF, --leftneighbours getrightneighbours as LEFT-NEIGHBOUR-OF,
 * --subsumed getsubparents as SUBSUMED-BY, --subsumes getsubchildren as SUBSUMES.
 * The two skipgram kinds look at the window [t, t + n(A)) only; a reference whose window leaves its sentence or the corpus has no rows (a
 * trained model has none; the reference reads past the sentence there). COLIBRI_REL_TEMPLATES drops A itself with the reference's comparison
 * of the masked corpus window against A's bytes AT THE SAME INDEX (src/pattern.cpp:1009-1041), under which a skipgram whose gap covers a
 * multi-byte token is listed as its own template.
 *   threshold t > 0: B must have a count >= t and the joint count must be >= t (prunerelations :3066-3078); t = 0: every row.
 *   COLIBRI_REL_TEMPLATES with t > 0: A's own count must be >= t and the joint count >= t; B's own count is not tested (as the reference).
 * Rows are ordered by A's pattern number, then count descending, then B's key bytes, ascending (the reference's order within a pattern is its
 * unordered_map's). Input = an indexed model in the layout colibri_export_indexed writes, the uploaded corpus is the reverse index; a flexgram in
 * the model is refused (COLIBRI_ERR_UNSUPPORTED). The result stays on the device until the next call; *nrows rows. Events are counted per A
 * occurrence first and processed in chunks of a fixed scratch budget, cut anywhere along the forward index; the partial counts of a pattern cut
 * by a chunk boundary are merged before the threshold (environment: COLIBRI_REL_CHUNK = events per chunk). */
enum { COLIBRI_REL_SUBCHILDREN = 0, COLIBRI_REL_SUBPARENTS = 1, COLIBRI_REL_LEFTNEIGHBOURS = 2, COLIBRI_REL_RIGHTNEIGHBOURS = 3, COLIBRI_REL_INSTANCES = 4, COLIBRI_REL_TEMPLATES = 5 };
int colibri_relations(colibri_ctx* ctx, const uint64_t* key_off, const uint8_t* key_bytes, const uint64_t* ref_off, const uint32_t* ref_sentence, const uint16_t* ref_token,
                      uint64_t npatterns, int kind, uint32_t threshold, uint64_t* nrows);
/* The same on the indexed model of the last colibri_train of this context, still resident in HBM (pattern numbers = colibri_export_indexed's).
 * COLIBRI_ERR_STATE unless the context holds a trained indexed model of a non-sharded run. */
int colibri_relations_resident(colibri_ctx* ctx, int kind, uint32_t threshold, uint64_t* nrows);
/* the rows, into caller-allocated arrays of nrows entries (any may be NULL): pattern numbers of A and B, count */
int colibri_relations_fetch(colibri_ctx* ctx, uint32_t* pattern_a, uint32_t* pattern_b, uint32_t* counts);
/* what the last call did: related occurrences (events), chunks, the peak of the scratch the call takes itself (as colibri_cooc_info) */
int colibri_relations_info(const colibri_ctx* ctx, uint64_t* events, uint64_t* chunks, uint64_t* scratch_bytes);

/* ---- skip content of an indexed model's skipgrams (colibri-patternmodeller --skipcontent) ---------------------------------------------------
 * Replaces the reference's per-pattern loop IndexedPatternModel::getskipcontent (include/patternmodel.h:3029-3059) run over every pattern A of
 * the model. Only an A with a gap has rows. With n = n(A), head = the index of A's first gap and tail = the tokens after its last gap, each
 * reference (s, t) of A in A's own forward index yields the corpus bytes of the tokens [t + head, t + n - tail) of sentence s: the mask is
 * dropped, so the tokens between two gaps are part of the content. One row per (A, distinct content) with its count; no threshold. A reference
 * whose window [t, t + n) leaves its sentence or the corpus is skipped (counted in skipped_refs; a trained model has none; the reference reads
 * past the sentence there). A content is no pattern of the model: its identity is its bytes, decided on the device by byte checks against a
 * representative reference, never by a hash (environment: COLIBRI_SKC_HASH_BITS = 1..63 narrows the hash, so that the checks and the further
 * rounds for true collisions do the work). Each row also carries the content's pattern number in the model when the model holds that n-gram,
 * else 0xFFFFFFFF (the CLI prints COUNT2 from it). Rows are ordered by A's pattern number, then count descending, then the content's bytes
 * ascending (byte-lexicographic, a proper prefix first). Input, state rules, refusals (a flexgram: COLIBRI_ERR_UNSUPPORTED) and chunking
 * (COLIBRI_REL_CHUNK) as colibri_relations. *nrows rows, *content_bytes = the bytes of all rows' contents. */
int colibri_skipcontent(colibri_ctx* ctx, const uint64_t* key_off, const uint8_t* key_bytes, const uint64_t* ref_off, const uint32_t* ref_sentence, const uint16_t* ref_token,
                        uint64_t npatterns, uint64_t* nrows, uint64_t* content_bytes);
int colibri_skipcontent_resident(colibri_ctx* ctx, uint64_t* nrows, uint64_t* content_bytes);
/* the rows, into caller-allocated arrays (any may be NULL): pattern number of A, the content's pattern number in the model or 0xFFFFFFFF, count
 * (nrows entries each), content_off (nrows + 1 offsets into content_bytes), content_bytes */
int colibri_skipcontent_fetch(colibri_ctx* ctx, uint32_t* pattern_a, uint32_t* pattern_b, uint32_t* counts, uint64_t* content_off, uint8_t* content_bytes);
/* what the last call did: events (references with a content), chunks, the peak of the scratch the call takes itself, identity rounds (1 unless
 * two different contents shared a hash), references skipped because their window leaves the sentence */
int colibri_skipcontent_info(const colibri_ctx* ctx, uint64_t* events, uint64_t* chunks, uint64_t* scratch_bytes, uint64_t* rounds, uint64_t* skipped_refs);

/* ---- log-likelihood comparison of pattern models (colibri-comparemodels) -------------------------------------------------------------------
 * The reference's comparemodels_loglikelihood over whole models (src/patternmodel.cpp:22-171, Rayson & Garside 2000). Input: nmodels >= 2
 * models, each as key_off[m] (npatterns[m] + 1 offsets) / key_bytes[m] / counts[m] (npatterns[m]), and tokens[m] = the model's tokens(); a
 * model of more than INT_MAX tokens is refused (COLIBRI_ERR_OVERFLOW). Rows = the distinct patterns of all models, identified by their key
 * bytes (COLIBRI_COMPARE_CONJUNCTION: only those with a non-zero count in every model). Per row, with o_i its count in model i and n_i = tokens[i]:
 *   e_i = exp(log(n_i) + log(sum o) - log(sum n)),  ll = 2 * sum over o_i > 0 of o_i * log(o_i / e_i),  NaN -> 0,
 * in double on the device (log / exp need not match glibc bit for bit). Rows are ordered by ll descending, then key bytes ascending (a proper
 * prefix first); COLIBRI_COMPARE_UNSORTED keeps them in the order of their first occurrence (model, then index). The result stays on the device
 * until the next call; *nrows rows. Environment: COLIBRI_COMPARE_HASH_BITS = b keeps b bits of the key hash (tests: identity by the bytes). */
enum { COLIBRI_COMPARE_CONJUNCTION = 1, COLIBRI_COMPARE_UNSORTED = 2 };
int colibri_compare(colibri_ctx* ctx, int nmodels, const uint64_t* const* key_off, const uint8_t* const* key_bytes, const uint32_t* const* counts, const uint64_t* npatterns,
                    const uint64_t* tokens, int flags, uint64_t* nrows);
/* the rows, into caller-allocated arrays (any may be NULL): a representative occurrence of each row (model[r], index[r] = the pattern's number
 * in that model's input, the first model that holds it), ll[r], and nrows x nmodels arrays: observed[r * nmodels + i] = the row's count in model
 * i (0: absent), group_totals[r * nmodels + i] = model i's occurrences of the row's (category, size) group as unsigned int (0 for a flexgram) */
int colibri_compare_fetch(colibri_ctx* ctx, uint32_t* model, uint32_t* index, double* ll, uint32_t* observed, uint32_t* group_totals);
/* what the last call did: distinct patterns (before the conjunction filter), the peak of the scratch it took itself (the uploaded models included;
 * not counted: the context's radix-sort buffers and the result arrays) */
int colibri_compare_info(const colibri_ctx* ctx, uint64_t* distinct, uint64_t* scratch_bytes);

/* ---- corpus decoding (colibri-classdecode) --------------------------------------------------------------------------------------------------
 * The reference's ClassDecoder::decodefile (src/classdecoder.cpp:166-238): a class-encoded corpus back to text, the specification in
 * csrc/decode.hpp and DESIGN.md §5d. Three steps:
 *   colibri_decode_upload   the corpus WITHOUT its A2 <version> header; version 1 = header-less v1 data (length-prefixed base-256 ids, 128 / 129
 *                           = the {*} / {**} markers), converted on the host; anything else = v2 varints. It replaces the context's corpus (a
 *                           training run needs a new colibri_upload_corpus) and reports the highest id of a word token. Refused: more than
 *                           ingest's 4 GiB (COLIBRI_ERR_CORPUS), and in v2 a token of more than 5 bytes or a multi-byte token of id 0.
 *   colibri_decode_classes  the word table: nids + 1 offsets into word_bytes, the word of id k = word_bytes[word_off[k] .. word_off[k + 1]); an id
 *                           without a word has length 0, and so has every id >= nids. At most 2^26 ids (COLIBRI_ERR_OVERFLOW beyond).
 *   colibri_decode          the text of lines end < L < start hidden as the reference hides them (start = end = 0: every line), handed to
 *                           sink(user, p, n) in consecutive pieces of at most one window (COLIBRI_DECODE_WINDOW_BYTES, default 64 MiB); a non-zero
 *                           return of the sink stops the call with COLIBRI_ERR_STATE. *outbytes = the text's length, *nlines = the 00 tokens (the
 *                           reference's "Processed <n> lines"). The pieces point into pinned buffers of the context, valid during the call only. */
typedef int (*colibri_decode_sink)(void* user, const uint8_t* p, uint64_t n);
int colibri_decode_upload(colibri_ctx* ctx, const uint8_t* payload, uint64_t nbytes, int version, uint64_t* maxclass);
int colibri_decode_classes(colibri_ctx* ctx, const uint64_t* word_off, const uint8_t* word_bytes, uint64_t nids);
int colibri_decode(colibri_ctx* ctx, uint32_t start, uint32_t end, colibri_decode_sink sink, void* user, uint64_t* outbytes, uint64_t* nlines);
/* what the last colibri_decode did: output windows, bytes of pinned host staging (two windows), the peak of the device scratch it took */
int colibri_decode_info(const colibri_ctx* ctx, uint64_t* windows, uint64_t* staging_bytes, uint64_t* scratch_bytes);

/* ---- coverage report of a pattern model (colibri-patternmodeller -R / -r) ---------------------------------------------------------------------
 * Replaces the loops of computestats (reference include/patternmodel.h:1903-1935) and computecoveragestats (:1946-1995, :3390-3450); the
 * specification is in csrc/coverage.hpp and DESIGN.md §5e. Groups are (category c, size n), c in {0 = all, 1 = n-gram, 2 = skipgram,
 * 3 = flexgram}, n in {0 = all, 1 .. maxn} with n = Pattern::n() (a gap is one token). *ngroups_n = G = maxn + 1 (0 for an empty model); the
 * result is four arrays of 4 * G values, group (c, n) at c * G + n:
 *   patterns, counts  patterns of the group and the sum of their counts; a flexgram is in (0, 0) and (3, 0) only
 *   types             distinct class ids among the tokens of the group's patterns, gap markers included
 *   tokens            distinct corpus positions (sentence, (token + i) mod 65536), i < n, under the references of the group's patterns; for n > 0
 *                     only with COLIBRI_COV_PER_SIZE in flags (0 without it), and 0 everywhere when the model has no references
 * Input = a model in the layout colibri_export_indexed writes. counts may be NULL when ref_off is given (a pattern's count is then its number of
 * references); ref_off / ref_sentence / ref_token may be NULL for an unindexed model. No corpus has to be uploaded. What report() does with the
 * values (per-size token rows print 0, unindexed rows print the sum of all counts) is the host face's business.
 * COLIBRI_ERR_OVERFLOW when the sentence range of the references or the bitmaps exceed the scratch budget (environment: COLIBRI_COV_BUDGET =
 * bytes, default 8 GiB), or a token has more than 9 bytes. Environment: COLIBRI_COV_SLICE = references per block of the per-reference kernels. */
enum { COLIBRI_COV_PER_SIZE = 1, COLIBRI_COV_NO_TOKENS = 2 /* no reference is read: tokens stay 0 (computestats, the CLI's -r) */ };
int colibri_coverage(colibri_ctx* ctx, const uint64_t* key_off, const uint8_t* key_bytes, const uint32_t* counts, const uint64_t* ref_off, const uint32_t* ref_sentence,
                     const uint16_t* ref_token, uint64_t npatterns, int flags, uint64_t* ngroups_n);
/* The same on the indexed model of the last colibri_train of this context, still resident in HBM. COLIBRI_ERR_STATE unless the context holds a
 * trained indexed model of a non-sharded run. */
int colibri_coverage_resident(colibri_ctx* ctx, int flags, uint64_t* ngroups_n);
/* the values, into caller-allocated arrays of 4 * G entries (any may be NULL) */
int colibri_coverage_fetch(colibri_ctx* ctx, uint64_t* patterns, uint64_t* counts, uint64_t* types, uint64_t* tokens);
/* what the last call did: references marked, bytes of class and position bitmaps, the peak of the scratch the call took itself (as colibri_cooc_info) */
int colibri_coverage_info(const colibri_ctx* ctx, uint64_t* references, uint64_t* bitmap_bytes, uint64_t* scratch_bytes);

/* ---- the text and the histogram of a pattern model (colibri-patternmodeller -P / -H) --------------------------------------------------------------
 * Replaces the loops of PatternModel::print and histogram of the host face (reference include/patternmodel.h:2294-2441, :2930-2959); the
 * specification is in csrc/print.hpp and DESIGN.md §5f. Every row of print() — text, count, count x size, coverage, category, size, frequency and,
 * for an indexed model, its sentence:token references — is byte-equal to what the host loop writes on a stream in its default float state; the
 * header line and the legend stay with the caller. Rows come in the order of the arrays.
 *   colibri_print_classes   the word table, as colibri_decode_classes takes it, plus has_word: nids bytes, non-zero = the id has a word (an id
 *                           without one, and every id >= nids, prints {?}; an id with an empty word prints nothing). has_word NULL: every id
 *                           below nids has a word. At most 2^26 ids (COLIBRI_ERR_OVERFLOW beyond).
 *   colibri_print_model     a model in the layout colibri_export_indexed writes. counts may be NULL when ref_off is given (a pattern's count is
 *                           then its number of references); ref_off / ref_sentence / ref_token NULL: an unindexed model, rows without the
 *                           reference column. tokens = the model's tokens() (below 2^53). The text goes to sink(user, p, n) in consecutive pieces of
 *                           at most one window (COLIBRI_PRINT_WINDOW_BYTES, default 64 MiB), as colibri_decode hands its text over; a non-zero
 *                           return of the sink stops the call with COLIBRI_ERR_STATE. *outbytes = the text's length.
 *   colibri_print_model_resident  the same on the model of the last colibri_train of this context where it lies in HBM, indexed or not.
 *                           COLIBRI_ERR_STATE for an untrained context or a sharded run.
 * COLIBRI_ERR_OVERFLOW, with the context usable afterwards: scratch above the budget (COLIBRI_PRINT_BUDGET = bytes, default 8 GiB; 47 bytes per
 * pattern, 12 per reference, two windows), 2^32 references or more, a token of more than 9 bytes, a row of 4 GiB or more.
 * Environment: COLIBRI_PRINT_SLICE = references per block of the reference kernel (default 2048). */
int colibri_print_classes(colibri_ctx* ctx, const uint64_t* word_off, const uint8_t* word_bytes, const uint8_t* has_word, uint64_t nids);
int colibri_print_model(colibri_ctx* ctx, const uint64_t* key_off, const uint8_t* key_bytes, const uint32_t* counts, const uint64_t* ref_off, const uint32_t* ref_sentence,
                        const uint16_t* ref_token, uint64_t npatterns, uint64_t tokens, colibri_decode_sink sink, void* user, uint64_t* outbytes);
int colibri_print_model_resident(colibri_ctx* ctx, uint64_t tokens, colibri_decode_sink sink, void* user, uint64_t* outbytes);
/* print(..., instantiate = true) (colibri-patternmodeller -P --instantiate; reference include/patternmodel.h:2948-2959): the same rows, and in a skipgram
 * row of n tokens every reference s:t is followed by '[', the words of the n corpus tokens that start at (s, t), ']'. The corpus is the one this context
 * holds (colibri_upload_corpus; for the resident form the one the model was trained on), its sentences numbered from its first_sentence, empty ones
 * counted; COLIBRI_ERR_STATE without one. An unindexed model prints as colibri_print_model prints it. Arguments and the sink as above.
 *   COLIBRI_ERR_UNSUPPORTED  the model holds a flexgram (the reference's walk for it accepts gaps of exactly one token and aborts otherwise)
 *   COLIBRI_ERR_ARG          a skipgram's reference does not fit the corpus: its sentence is not in it, or ends before token + n (a model beside
 *                            another corpus). Found by the length pass, which reads nothing outside the corpus; the sink has not been called. */
int colibri_print_instances(colibri_ctx* ctx, const uint64_t* key_off, const uint8_t* key_bytes, const uint32_t* counts, const uint64_t* ref_off, const uint32_t* ref_sentence,
                            const uint16_t* ref_token, uint64_t npatterns, uint64_t tokens, colibri_decode_sink sink, void* user, uint64_t* outbytes);
int colibri_print_instances_resident(colibri_ctx* ctx, uint64_t tokens, colibri_decode_sink sink, void* user, uint64_t* outbytes);
/* what the last print call did: output windows, bytes of pinned host staging (two windows), the peak of the device scratch it took */
int colibri_print_info(const colibri_ctx* ctx, uint64_t* windows, uint64_t* staging_bytes, uint64_t* scratch_bytes);
/* The histogram: the distinct counts of the patterns of one group, ascending, and the number of patterns of each. category 0 = every category
 * (else Pattern::category(): 1 n-gram, 2 skipgram, 3 flexgram), size 0 = every size (else Pattern::size()). The references themselves are not
 * needed: ref_off alone gives an indexed model's counts. Threshold and cap are the caller's, over the *nrows pairs colibri_histogram_fetch copies
 * into caller-allocated arrays (either may be NULL). */
int colibri_histogram(colibri_ctx* ctx, const uint64_t* key_off, const uint8_t* key_bytes, const uint32_t* counts, const uint64_t* ref_off, uint64_t npatterns, int category,
                      uint64_t size, uint64_t* nrows);
int colibri_histogram_resident(colibri_ctx* ctx, int category, uint64_t size, uint64_t* nrows);
int colibri_histogram_fetch(colibri_ctx* ctx, uint32_t* counts, uint64_t* patterns);

/* ---- the reverse index (colibri-patternmodeller -Z, PatternModel::getreverseindex / printreverseindex) ---------------------------------------------
 * For every real token position (sentence, token) of the corpus uploaded with colibri_upload_corpus: the patterns of the model that start there
 * (reference include/patternmodel.h:1746-1824; the specification is in csrc/rindex.hpp and DESIGN.md §5g). A window of n tokens, MINLENGTH <= n <=
 * MAXLENGTH of the model, counts when the model has it; for n >= 3 the window under every gap mask a skipgram of the model has at that length
 * counts when the model has that key. occurrencecount > 0: only patterns with at least that count (counts: one per pattern; NULL only with
 * occurrencecount 0); category 0 = any, 1 n-grams, 2 skipgrams (3, flexgrams: nothing); size 0 = any length. Rows: positions ascending, within a
 * position n ascending, the n-gram before its skipgrams, masks ascending. The model may be indexed or not. A flexgram in the model is refused
 * (COLIBRI_ERR_UNSUPPORTED).
 *   colibri_rindex           a model's keys in the layout colibri_export_unindexed writes; *npositions = real token positions, *nrows = patterns
 *                            over all of them. The result stays on the device until the next call.
 *   colibri_rindex_resident  the same on the model of the last colibri_train of this context where it lies in HBM; pattern numbers are the
 *                            export order's. COLIBRI_ERR_STATE for an untrained context.
 *   colibri_rindex_fetch     pos_off (npositions + 1: the rows of position r are pattern[pos_off[r] .. pos_off[r + 1])), sentence and token of
 *                            every position (the sentence numbers start at the upload's first_sentence; empty sentences are counted), pattern
 *                            (nrows pattern numbers) into caller-allocated arrays; any may be NULL.
 *   colibri_rindex_text      printreverseindex's text of the last index: per position "s:t", then "\t<pattern text>" per pattern, then "\n"; one
 *                            more "\n" after the last line. The pattern text is colibri_print_model's, from the word table of
 *                            colibri_print_classes (it tells an id without a word, {?}, from an empty word). The text goes to sink(user, p, n) in
 *                            consecutive pieces of at most one window (COLIBRI_RINDEX_WINDOW_BYTES, default 64 MiB), as colibri_print_model hands
 *                            its text over. COLIBRI_ERR_STATE before an index call or without a word table.
 *   colibri_rindex_info      what the last calls did: position chunks of the index, output windows and pinned staging bytes of the text, the peak
 *                            of the device scratch.
 * COLIBRI_ERR_STATE without an uploaded corpus or on a sharded run. COLIBRI_ERR_OVERFLOW, with the context usable afterwards: scratch and result
 * above the budget (COLIBRI_RINDEX_BUDGET = bytes, default 8 GiB; the look-ups run over chunks of positions sized from it, 4 bytes x layers + 16
 * per position; COLIBRI_RINDEX_CHUNK = positions per chunk), 2^32 - 16 rows or more, a sentence of more than 65536 tokens, a line of 4 GiB or
 * more, a skipgram of more than 13 tokens. */
int colibri_rindex(colibri_ctx* ctx, const uint64_t* key_off, const uint8_t* key_bytes, const uint32_t* counts, uint64_t npatterns, uint32_t occurrencecount, int category,
                   uint64_t size, uint64_t* npositions, uint64_t* nrows);
int colibri_rindex_resident(colibri_ctx* ctx, uint32_t occurrencecount, int category, uint64_t size, uint64_t* npositions, uint64_t* nrows);
int colibri_rindex_fetch(colibri_ctx* ctx, uint64_t* pos_off, uint32_t* sentence, uint16_t* token, uint32_t* pattern);
int colibri_rindex_text(colibri_ctx* ctx, colibri_decode_sink sink, void* user, uint64_t* outbytes);
int colibri_rindex_info(const colibri_ctx* ctx, uint64_t* chunks, uint64_t* windows, uint64_t* staging_bytes, uint64_t* scratch_bytes);

/* ---- a model queried with new text (colibri-patternmodeller -q / --queryfile, PatternModel::getpatterns / query) -----------------------------------
 * Which patterns of the model occur in these lines, and where (reference src/patternmodeller.cpp:160-231, include/patternmodel.h:2272-2285; the
 * specification is in csrc/query.hpp and DESIGN.md §5i). The text is a payload in the layout colibri_upload_corpus takes, every line closed by the
 * delimiter byte, empty lines kept (tokens after the last delimiter form one more line); it is another text than the context's corpus, which,
 * like the trained model and its references, is only read. Line s (0-based) has the number first_line + s. exact: one byte per line (NULL: all
 * 0). A line with exact 0 (extensive mode), of pattern P and T tokens: the row (line, 0, P) when the model has P, whatever minlength and
 * maxlength; then for n = minlength .. min(maxlength, T) and token i = 0 .. T - n the row (line, i, window of n tokens at i) when the model has
 * that window — the whole-line row is repeated among them when T lies in that range. A line with exact != 0: one row (line, 0, P), with
 * pattern 0xFFFFFFFF when the model does not have P (also for a line of no tokens). A line of no tokens in extensive mode has no row. Identity
 * is equality of key bytes: gap markers are tokens like any other, so a skipgram or flexgram of the model matches only a line that has the
 * markers at the same places. Rows are line-major, the whole-line row first, then length-major, then by token: a function of the input alone.
 *   colibri_query           the model arrays are colibri_print_model's; counts and the reference arrays may be NULL under its rules, and both
 *                           counts and ref_off may be NULL when only the rows are wanted. *nlines = lines of the payload, *nrows = rows over all
 *                           of them. Pattern numbers are positions in the arrays. The result stays on the device until the next query call.
 *   colibri_query_resident  the same on the model of the last colibri_train of this context where it lies in HBM; pattern numbers are the
 *                           export order's. COLIBRI_ERR_STATE for an untrained context. The exports and colibri_rindex_resident answer
 *                           afterwards as before.
 *   colibri_query_fetch     line_off (nlines + 1: the rows of line s are [line_off[s], line_off[s + 1])), token and pattern of every row into
 *                           caller-allocated arrays; any may be NULL.
 *   colibri_query_text      the text of the last query: per row of extensive mode "L:i\t" and the row colibri_print_model writes for the pattern
 *                           (tokens = its tokens argument; the references of an indexed model included); per row of exact mode that row alone, or
 *                           PATTERN "<the line's text>" NOT FOUND IN MODEL and a newline. Words come from the table of colibri_print_classes. The
 *                           text goes to sink(user, p, n) in consecutive pieces of at most one window (COLIBRI_QUERY_WINDOW_BYTES, default
 *                           64 MiB), which may cut a row anywhere. COLIBRI_ERR_STATE before a query call, without a word table, for a model
 *                           given without counts and offsets, or when the resident model the query ran on has been replaced.
 *   colibri_query_info      what the last calls did: position chunks of the look-ups, output windows and pinned staging bytes of the text, the
 *                           peak of the device scratch.
 * COLIBRI_ERR_OVERFLOW, with the context usable afterwards: scratch and result above the budget (COLIBRI_QUERY_BUDGET = bytes, default 8 GiB; the
 * look-ups run over chunks of positions sized from it, 16 bytes x lengths + 4 per position; COLIBRI_QUERY_CHUNK = positions per chunk),
 * 2^32 - 16 rows or more, a line of more than 65536 tokens, a text line of 4 GiB or more. */
int colibri_query(colibri_ctx* ctx, const uint64_t* key_off, const uint8_t* key_bytes, const uint32_t* counts, const uint64_t* ref_off, const uint32_t* ref_sentence,
                  const uint16_t* ref_token, uint64_t npatterns, const uint8_t* payload, uint64_t nbytes, uint32_t first_line, const uint8_t* exact, int minlength,
                  int maxlength, uint64_t* nlines, uint64_t* nrows);
int colibri_query_resident(colibri_ctx* ctx, const uint8_t* payload, uint64_t nbytes, uint32_t first_line, const uint8_t* exact, int minlength, int maxlength, uint64_t* nlines,
                           uint64_t* nrows);
int colibri_query_fetch(colibri_ctx* ctx, uint64_t* line_off, uint16_t* token, uint32_t* pattern);
int colibri_query_text(colibri_ctx* ctx, uint64_t tokens, colibri_decode_sink sink, void* user, uint64_t* outbytes);
int colibri_query_info(const colibri_ctx* ctx, uint64_t* chunks, uint64_t* windows, uint64_t* staging_bytes, uint64_t* scratch_bytes);

/* ---- the subsumption prunes of a finished model (colibri-patternmodeller -p / --prunesubsumed, PRUNENONSUBSUMED / PRUNESUBSUMED) ------------------
 * Which patterns of the model survive the two post-hoc prunes of train() (reference include/patternmodel.h:1285-1336; the specification is in
 * csrc/subsume.hpp and DESIGN.md §5j). The sub-patterns of a pattern of n tokens are its first and its last n - 1 tokens ({*} is a token). Pass 1
 * (prunenonsubsumed = p > 0), n = min(p, maxlength) down to 2: when any pattern of n tokens is alive, every alive pattern of n - 1 tokens that is
 * no sub-pattern of one of them dies; a level without alive n-token patterns does nothing. Pass 2 (prunesubsumed = S > 0), on pass 1's survivors,
 * n = 2 up to min(S, maxlength): every alive pattern of n - 1 tokens that is a sub-pattern of an alive pattern of n tokens dies. Only the keys are
 * read: counts and references stay the caller's, who compacts its arrays by the flags. No corpus is needed.
 *   colibri_subsume           the keys are colibri_print_model's key arrays. *nkept = patterns left.
 *   colibri_subsume_resident  the same on the model of the last colibri_train of this context where it lies in HBM, which stays as it is;
 *                             *npatterns = its patterns, the flags are in export order. COLIBRI_ERR_STATE for an untrained context.
 *   colibri_subsume_fetch     keep (npatterns bytes, 1 = the pattern survives, in the order of the arrays) and the patterns each pass pruned, by
 *                             the tokens of the pruned patterns (COLIBRI_MAX_ORDER entries each); any may be NULL. COLIBRI_ERR_STATE before a call.
 *   colibri_subsume_info      what the last call did: levels whose marking patterns were looked up, sub-pattern look-ups (two per alive marking
 *                             pattern), the peak of the device scratch.
 * COLIBRI_ERR_ARG for a negative argument, COLIBRI_ERR_UNSUPPORTED for a model that holds a flexgram, COLIBRI_ERR_OVERFLOW for levels above
 * COLIBRI_MAX_ORDER tokens. COLIBRI_SUBSUME_HASH_BITS = bits (tests): that many bits of the key hash, so that the byte check decides identity. */
int colibri_subsume(colibri_ctx* ctx, const uint64_t* key_off, const uint8_t* key_bytes, uint64_t npatterns, int prunenonsubsumed, int prunesubsumed, int maxlength, uint64_t* nkept);
int colibri_subsume_resident(colibri_ctx* ctx, int prunenonsubsumed, int prunesubsumed, int maxlength, uint64_t* npatterns, uint64_t* nkept);
int colibri_subsume_fetch(colibri_ctx* ctx, uint8_t* keep, uint64_t* pruned_non, uint64_t* pruned_sub);
int colibri_subsume_info(const colibri_ctx* ctx, uint64_t* levels, uint64_t* probes, uint64_t* scratch_bytes);

/* ---- the skipgrams of an in-place rebuild (colibri-patternmodeller -I -s, PatternModel::trainskipgrams_selfconstrained) -----------------------------
 * Counts given skipgrams on the uploaded corpus (reference include/patternmodel.h:1569-1604; the specification is in csrc/recount.hpp and
 * DESIGN.md §5k). A skipgram of n >= 3 tokens with gap mask m occurs at (s, t) iff t + n <= sentencelength(s) and every token outside m equals
 * the key's: a gap takes any one token, a window never crosses a sentence end. MINSKIPTYPES, MINTOKENS_SKIPGRAMS and MAXSKIPS play no part.
 *   colibri_recount        the keys are colibri_print_model's key arrays and have to be skipgrams. indexed != 0: the references are kept too.
 *                          mintokens (0 counts as 1): *nkept = the keys whose count reaches it, *nrefs = their references (0 for an unindexed call).
 *   colibri_recount_fetch  into caller-allocated arrays aligned to the keys (any may be NULL): counts (npatterns; the true count, also below
 *                          mintokens) and, of an indexed call, ref_off (npatterns + 1) and the references (nrefs each): every run ascends by
 *                          (sentence, token), sentences numbered from colibri_upload_corpus's first_sentence; a key below mintokens has an empty
 *                          run. COLIBRI_ERR_STATE before a call.
 *   colibri_recount_info   what the last call did: (length, mask) groups, position chunks, the peak of the device scratch.
 * With the context usable afterwards: COLIBRI_ERR_STATE without a corpus; COLIBRI_ERR_UNSUPPORTED for a key that is not a skipgram of three or
 * more tokens, a flexgram, a skipgram of more than 13 tokens, a corpus with a sentence of 65536 tokens or more; COLIBRI_ERR_OVERFLOW for scratch
 * and result above the budget (COLIBRI_RECOUNT_BUDGET = bytes, default 8 GiB; the look-ups run over chunks of positions sized from it, 4 bytes x
 * groups + 16 per position; COLIBRI_RECOUNT_CHUNK = positions per chunk) or 2^32 - 16 references or more. */
int colibri_recount(colibri_ctx* ctx, const uint64_t* key_off, const uint8_t* key_bytes, uint64_t npatterns, int indexed, uint32_t mintokens, uint64_t* nkept, uint64_t* nrefs);
int colibri_recount_fetch(colibri_ctx* ctx, uint32_t* counts, uint64_t* ref_off, uint32_t* ref_sentence, uint16_t* ref_token);
int colibri_recount_info(const colibri_ctx* ctx, uint64_t* groups, uint64_t* chunks, uint64_t* scratch_bytes);

/* ---- the skipgrams of an indexed model that holds its n-grams (colibri-patternmodeller -i model -s, IndexedPatternModel::trainskipgrams) -----------
 * Replaces reference include/patternmodel.h:2969-3010 (the specification is in csrc/modelskip.hpp and DESIGN.md §5m). No corpus is read. With
 * t = mintokens (-1: 2) and msk = max(mintokens_skipgrams, t), for n = 3 .. maxlength and the gap masks of compute_skip_configurations(n, maxskips):
 * every n-gram of n tokens (msk > 1: whose first and last n - 1 tokens are both still patterns of the model) gives one candidate per mask, its key
 * with every masked token replaced by the byte 03; equal candidates are one skipgram, count = the sum of its sources' reference counts, types =
 * its sources. An order without a skipgram ends the loop unpruned; otherwise every pattern of n tokens below t goes, n-grams too (the next order
 * sees that), then every skipgram with fewer than minskiptypes types (minskiptypes > 1).
 *   colibri_modelskip           the model in colibri_print_model's layout with its forward index. *nskipgrams / *keybytes / *nrefs: the totals of
 *                               the kept skipgrams, what the fetch's arrays must hold; *nerased: the model's own patterns that go.
 *   colibri_modelskip_resident  the same on the indexed model of the last colibri_train of this context where it lies in HBM, which stays as it is.
 *   colibri_modelskip_fetch     key_off / ref_off (nskipgrams + 1), key_bytes, counts and types (nskipgrams), the references (nrefs; every list
 *                               ascends by (sentence, token)) and keep (one byte per pattern of the model, in the order of its arrays: 1 = it stays;
 *                               may be NULL). The skipgrams come by order, within an order by their first candidate (source ascending, then mask).
 *   colibri_modelskip_info      what the last call did: *orders orders were looked at, 3 .. *orders + 2 (the last may have found nothing: the loop
 *                               ended there); found / pruned / extra: COLIBRI_MAX_ORDER entries by the order n (pruned counts n-grams and
 *                               skipgrams below t, as the reference's progress line does); candidates; the peak of the device scratch.
 * With the context usable afterwards: COLIBRI_ERR_UNSUPPORTED for a model that holds a skipgram or a flexgram already (a 03 or 04 token) or a
 * source n-gram of more than 31 tokens; COLIBRI_ERR_OVERFLOW for 2^32 - 16 or more candidates or kept references in one order (they are not
 * chunked) and for hash collisions under four seeds. COLIBRI_MSKIP_HASH_BITS = bits[:attempts] (tests): that many bits of the group hash during
 * the first attempts (default 3) of the four, so that the byte compares and the retries run. */
int colibri_modelskip(colibri_ctx* ctx, const uint64_t* key_off, const uint8_t* key_bytes, const uint64_t* ref_off, const uint32_t* ref_sentence, const uint16_t* ref_token,
                      uint64_t npatterns, int mintokens, int mintokens_skipgrams, int minskiptypes, int maxlength, int maxskips, uint64_t* nskipgrams, uint64_t* keybytes,
                      uint64_t* nrefs, uint64_t* nerased);
int colibri_modelskip_resident(colibri_ctx* ctx, int mintokens, int mintokens_skipgrams, int minskiptypes, int maxlength, int maxskips, uint64_t* nskipgrams, uint64_t* keybytes,
                               uint64_t* nrefs, uint64_t* nerased);
int colibri_modelskip_fetch(colibri_ctx* ctx, uint64_t* key_off, uint8_t* key_bytes, uint32_t* counts, uint32_t* types, uint64_t* ref_off, uint32_t* ref_sentence,
                            uint16_t* ref_token, uint8_t* keep);
int colibri_modelskip_info(const colibri_ctx* ctx, uint32_t* orders, uint64_t* found, uint64_t* pruned, uint64_t* extra, uint64_t* candidates, uint64_t* scratch_bytes);

/* N-gram extraction (colibri-extractngrams; reference src/extractngrams.cpp; csrc/ngrams.hpp): every window of n tokens inside a
 * line of a corpus as text, one per row, in corpus order. Nothing is counted and nothing pruned.
 *   colibri_ngrams       over the corpus of the last colibri_decode_upload (version 2 only: COLIBRI_ERR_UNSUPPORTED for an upload made with version
 *                        1) and the word table of the last colibri_print_classes (an id without a word prints {?}); COLIBRI_ERR_STATE without
 *                        either, the message names which. For each line of T tokens and i = 0 .. T - n: the words of the tokens i .. i + n - 1,
 *                        joined as colibri_print_model joins a pattern's, and a newline. The text goes to sink(user, p, n) in pieces of at most
 *                        one window (COLIBRI_NGRAMS_WINDOW_BYTES, default 64 MiB), which may cut a row anywhere; a non-zero return of the sink
 *                        stops the call with COLIBRI_ERR_STATE. *outbytes = the text's length, *nngrams = its rows (both 0 after a refusal).
 *                        COLIBRI_ERR_ARG for n == 0 or a NULL sink; COLIBRI_ERR_OVERFLOW for a word or a row of 4 MiB or more. The context stays
 *                        usable after every refusal.
 *   colibri_ngrams_info  what the last colibri_ngrams did: output windows, bytes of pinned host staging (two windows), the peak of the device scratch */
int colibri_ngrams(colibri_ctx* ctx, uint32_t n, colibri_decode_sink sink, void* user, uint64_t* outbytes, uint64_t* nngrams);
int colibri_ngrams_info(const colibri_ctx* ctx, uint64_t* windows, uint64_t* staging_bytes, uint64_t* scratch_bytes);

#ifdef __cplusplus
}
#endif
#endif
