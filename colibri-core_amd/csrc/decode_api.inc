// decode_api.inc — part of colibri_hip.hip (included there, inside its extern "C" block, after compare_api.inc): corpus decoding
// (colibri-classdecode; kernels and the specification in decode.hpp).

extern "C++" {
namespace {
// v1 data (reference src/classdecoder.cpp:204-238) as varints: a token = length byte 1..127 + that many little-endian base-256 digits (the
// first four count); 00 ends a line; 128 / 129 become the marker tokens of decode.hpp; bytes >= 130 are dropped; a token cut off by the end
// of the data is dropped. A token of id 0 becomes 80 00: in v1 it is a word (class 0's), not the end of a line.
std::vector<uint8_t> decode_v1_to_v2(const uint8_t* in, uint64_t n) {
    std::vector<uint8_t> out;
    out.reserve(n + n / 4);
    for (uint64_t i = 0; i < n;) {
        const uint8_t c = in[i];
        if (c == 0) {
            out.push_back(0);
            ++i;
        } else if (c < 128) {
            if (i + 1 + c > n) break;
            uint32_t cls = 0;
            for (unsigned k = 0; k < c && k < 4; ++k) cls |= (uint32_t)in[i + 1 + k] << (8 * k);
            if (cls == 0) {
                out.push_back(0x80);
                out.push_back(0);
            }
            while (cls) {
                const uint8_t b = cls & 127;
                cls >>= 7;
                out.push_back(cls ? (uint8_t)(b | 128) : b);
            }
            i += (uint64_t)c + 1;
        } else {
            if (c == 128 || c == 129) {
                out.insert(out.end(), c == 128 ? kDecodeSkipLen - 1 : kDecodeFlexLen - 1, (uint8_t)0x80);
                out.push_back(0);
            }
            ++i;
        }
    }
    return out;
}

// The output pump of colibri_decode and colibri_ngrams: `total` bytes of text leave in windows of B = min(env `var` or dflt, total) bytes. launch(W0, W1, stage)
// enqueues on c->stream whatever writes the text [W0, W1) to stage[q - W0]; the device writes window w into stage[w & 1] and copies it to pinned[w & 1] while the
// host hands window w - 1 to the sink. The pinned buffers and events are the context's (c->dc); the two stages are taken from S. A non-zero return of the sink
// stops the pump with COLIBRI_ERR_STATE ("<what>: the sink stopped the <verb> ..."). *windows / *staging: what was done, set when all of it was.
template <class Launch>
int pump_windows(colibri_ctx* c, DevScratch& S, const char* what, const char* verb, const char* var, uint64_t dflt, unsigned long long total, colibri_decode_sink sink, void* user,
                 Launch launch, uint64_t* windows, uint64_t* staging) {
    auto&          d = c->dc;
    const uint64_t B = std::min<uint64_t>(env_u64(var, dflt), total);  // (tests: windows of a few bytes, so that their edges fall inside lines and words)
    if (d.pinned_n < B) {
        for (auto& p : d.pinned) {
            if (p) (void)hipHostFree(p);
            p = nullptr;
        }
        d.pinned_n = 0;
        for (auto& p : d.pinned) HIP_TRY(c, hipHostMalloc(reinterpret_cast<void**>(&p), B, hipHostMallocDefault));
        d.pinned_n = B;
    }
    for (auto& e : d.ev)
        if (!e) HIP_TRY(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    DevBuf<uint8_t> stage[2];
    int             rc;
    if ((rc = S.take(stage[0], B)) || (rc = S.take(stage[1], B))) return rc;
    const uint64_t nw = (total + B - 1) / B;
    auto hand_over = [&](uint64_t w) -> int {
        HIP_TRY(c, hipEventSynchronize(d.ev[w & 1]));
        const uint64_t n = std::min<uint64_t>(B, total - w * B);
        if (const int s = sink(user, d.pinned[w & 1], n))
            return fail(c, COLIBRI_ERR_STATE, "%s: the sink stopped the %s (it returned %d) after %llu bytes", what, verb, s, (unsigned long long)(w * B));
        return COLIBRI_OK;
    };
    for (uint64_t w = 0; w < nw; ++w) {
        const unsigned long long W0 = w * B, W1 = std::min<uint64_t>(total, W0 + B);
        launch(W0, W1, stage[w & 1].p);
        HIP_TRY(c, hipMemcpyAsync(d.pinned[w & 1], stage[w & 1].p, W1 - W0, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipEventRecord(d.ev[w & 1], c->stream));
        if (w > 0 && (rc = hand_over(w - 1))) {
            (void)hipStreamSynchronize(c->stream);
            return rc;
        }
    }
    if ((rc = hand_over(nw - 1))) return rc;
    HIP_TRY(c, hipGetLastError());
    *windows = nw;
    *staging = 2 * B;
    return COLIBRI_OK;
}
}  // namespace
}  // extern "C++"

int colibri_decode_upload(colibri_ctx* c, const uint8_t* payload, uint64_t nbytes, int version, uint64_t* maxclass) {
    if (!c || (!payload && nbytes)) return COLIBRI_ERR_ARG;
    auto& d = c->dc;
    d.ready = false;
    std::vector<uint8_t> conv;
    const bool           v1 = version == 1;
    if (v1) {
        if (nbytes >= 0xFFFFFF00ull)  // (ingest's limit, on the input as given)
            return fail(c, COLIBRI_ERR_CORPUS, "corpus shard of %llu bytes exceeds the 4 GiB per-device limit (32-bit byte offsets); shard it", (unsigned long long)nbytes);
        conv    = decode_v1_to_v2(payload, nbytes);
        payload = conv.data();
        nbytes  = conv.size();
    }
    int rc = ingest(c, payload, nbytes, 1, hipMemcpyHostToDevice, false);
    c->have_corpus = false;  // (what the trainer refuses — a {**} token, say — is decoded; a training run uploads its corpus itself)
    c->trained     = false;
    if (rc) return rc;
    if (c->flags & kFlagTokenTooLong) return fail(c, COLIBRI_ERR_CORPUS, "decode: the corpus has a token of more than 8 bytes (an id beyond 32 bits)");
    if ((rc = dev_alloc(c, d.info, 1))) return rc;
    HIP_TRY(c, hipMemsetAsync(d.info.p, 0, sizeof(DecodeInfo), c->stream));
    if (c->npos) hipLaunchKernelGGL(decode_classify_kernel, dim3(blocks_for(c->npos, kBlock)), dim3(kBlock), 0, c->stream, c->bytes.p, c->tokstart.p, c->cls.p, c->npos, (int)v1, d.info.p);
    DecodeInfo h{};
    HIP_TRY(c, hipMemcpyAsync(&h, d.info.p, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    if (h.bad & kDecodeBadLong) return fail(c, COLIBRI_ERR_CORPUS, "decode: the corpus has a token of more than 5 bytes (an id beyond 32 bits)");
    if (h.bad & kDecodeBadZero) return fail(c, COLIBRI_ERR_CORPUS, "decode: the corpus has a multi-byte token of id 0, which no encoder writes");
    d.maxclass = h.maxclass;
    d.v1       = v1;
    d.ready    = true;
    if (maxclass) *maxclass = h.maxclass;
    return COLIBRI_OK;
}

int colibri_decode_classes(colibri_ctx* c, const uint64_t* word_off, const uint8_t* word_bytes, uint64_t nids) {
    if (!c || !word_off) return COLIBRI_ERR_ARG;
    auto& d = c->dc;
    d.nids  = 0;
    d.table = false;
    if (nids > kDecodeMaxIds)
        return fail(c, COLIBRI_ERR_OVERFLOW, "decode: a word table of %llu ids exceeds the bound of %u ids (the highest id that can have a word is %u)", (unsigned long long)nids,
                    kDecodeMaxIds, kDecodeMaxIds - 1);
    if (!word_bytes && word_off[nids] > word_off[0]) return COLIBRI_ERR_ARG;
    std::vector<uint32_t> off32(nids + 1, 0);
    for (uint64_t k = 1; k <= nids; ++k) {
        if (word_off[k] < word_off[k - 1]) return fail(c, COLIBRI_ERR_ARG, "decode: word offsets decrease at id %llu", (unsigned long long)k);
        if (word_off[k] - word_off[0] >= 0xFFFFFFFFull) return fail(c, COLIBRI_ERR_OVERFLOW, "decode: the words take 4 GiB or more (32-bit offsets)");
        off32[k] = (uint32_t)(word_off[k] - word_off[0]);
    }
    HIP_TRY(c, hipSetDevice(c->device));
    int rc;
    if ((rc = dev_alloc(c, d.wordoff, nids + 1)) || (rc = dev_alloc(c, d.words, (size_t)off32[nids] + 1))) return rc;
    HIP_TRY(c, hipMemcpyAsync(d.wordoff.p, off32.data(), sizeof(uint32_t) * (nids + 1), hipMemcpyHostToDevice, c->stream));
    if (off32[nids]) HIP_TRY(c, hipMemcpyAsync(d.words.p, word_bytes + word_off[0], off32[nids], hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // (the caller's arrays may go once this returns)
    d.nids  = (uint32_t)nids;
    d.table = true;
    return COLIBRI_OK;
}

int colibri_decode(colibri_ctx* c, uint32_t start, uint32_t end, colibri_decode_sink sink, void* user, uint64_t* outbytes, uint64_t* nlines) {
    if (!c || !sink) return COLIBRI_ERR_ARG;
    auto& d = c->dc;
    if (!d.ready) return fail(c, COLIBRI_ERR_STATE, "decode: no corpus uploaded by colibri_decode_upload");
    if (!d.table) return fail(c, COLIBRI_ERR_STATE, "decode: no word table installed by colibri_decode_classes");
    d.windows = d.staging = d.scratch = 0;
    if (outbytes) *outbytes = 0;
    if (nlines) *nlines = c->ndelim;  // "Processed <n> lines": the 00 tokens (src/classdecoder.cpp:196-197)
    const uint32_t npos = c->npos;
    if (npos == 0) return COLIBRI_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    // the hidden lines, end < L < start, as a run of positions [h0, h1)
    uint32_t h0 = npos, h1 = npos;
    if (!(start == 0 && end == 0) && (uint64_t)start > (uint64_t)end + 1) {
        auto line_start = [&](uint64_t L, uint32_t& pos) -> int {  // first position of line L (npos past the last one)
            pos = L == 1 ? 0u : npos;
            if (L == 1 || L - 2 >= c->ndelim) return COLIBRI_OK;
            HIP_TRY(c, hipMemcpy(&pos, c->delimpos.p + (L - 2), sizeof pos, hipMemcpyDeviceToHost));
            pos += 1;
            return COLIBRI_OK;
        };
        int rc;
        if ((rc = line_start((uint64_t)end + 1, h0)) || (rc = line_start(start, h1))) return rc;
    }
    const int                  v1 = d.v1 ? 1 : 0;
    DevScratch                 S{c};
    DevBuf<uint32_t>           len, range;
    DevBuf<unsigned long long> off, bsum;
    const uint32_t             nb = blocks_for(npos, kBlock * 4);
    int                        rc;
    if ((rc = S.take(len, npos)) || (rc = S.take(off, (size_t)npos + 1)) || (rc = S.take(bsum, nb)) || (rc = S.take(range, 2))) return rc;
    hipLaunchKernelGGL(decode_len_kernel, dim3(blocks_for(npos, kBlock)), dim3(kBlock), 0, c->stream, c->bytes.p, c->tokstart.p, c->cls.p, npos, v1, d.wordoff.p, d.nids, h0, h1,
                       len.p);
    hipLaunchKernelGGL(scan_reduce_kernel, dim3(nb), dim3(kBlock), 0, c->stream, len.p, npos, bsum.p);
    hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(kBlock), 0, c->stream, bsum.p, nb, off.p + npos);
    hipLaunchKernelGGL(scan_apply_kernel, dim3(nb), dim3(kBlock), 0, c->stream, len.p, npos, bsum.p, off.p);
    unsigned long long total = 0;
    HIP_TRY(c, hipMemcpyAsync(&total, off.p + npos, sizeof total, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    S.drop(len);
    S.drop(bsum);
    d.scratch = S.peak;
    if (total == 0) return COLIBRI_OK;
    rc = pump_windows(
        c, S, "decode", "decode", "COLIBRI_DECODE_WINDOW_BYTES", kDecodeWindowBytes, total, sink, user,
        [&](unsigned long long W0, unsigned long long W1, uint8_t* stage) {
            hipLaunchKernelGGL(decode_range_kernel, dim3(1), dim3(kWave), 0, c->stream, off.p, npos, W0, W1, range.p);
            hipLaunchKernelGGL(decode_write_kernel, dim3(stream_grid(npos)), dim3(kBlock), 0, c->stream, c->bytes.p, c->tokstart.p, c->cls.p, off.p, v1, d.wordoff.p, d.words.p, range.p,
                               W0, W1, stage);
        },
        &d.windows, &d.staging);
    d.scratch = S.peak;
    if (rc) return rc;
    if (outbytes) *outbytes = total;
    return COLIBRI_OK;
}

int colibri_decode_info(const colibri_ctx* c, uint64_t* windows, uint64_t* staging_bytes, uint64_t* scratch_bytes) {
    if (!c) return COLIBRI_ERR_ARG;
    if (windows) *windows = c->dc.windows;
    if (staging_bytes) *staging_bytes = c->dc.staging;
    if (scratch_bytes) *scratch_bytes = c->dc.scratch;
    return COLIBRI_OK;
}
