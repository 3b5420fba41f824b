// expand_api.inc — part of colibri_hip.hip (included there, inside its extern "C" block): colibri_set_seed, colibri_seed_fetch (expand.hpp; the seeded
// order loop itself is train_seeded in train_api.inc)
int colibri_set_seed(colibri_ctx* c, const uint64_t* key_off, const uint8_t* key_bytes, const uint32_t* counts, uint64_t npatterns) {
    if (!c) return COLIBRI_ERR_ARG;
    if (npatterns >= kMaxSeeds) return fail(c, COLIBRI_ERR_OVERFLOW, "seed set too large (at most 2^31 - 16 patterns)");
    if (npatterns && (!key_off || !key_bytes || !counts)) return COLIBRI_ERR_ARG;
    std::vector<uint8_t> order((size_t)npatterns);
    uint64_t             orders[2] = {0, 0};
    for (uint64_t p = 0; p < npatterns; ++p) {
        uint32_t ntok = 0;
        for (uint64_t k = key_off[p]; k < key_off[p + 1]; ++k) {
            const bool first = k == key_off[p] || key_bytes[k - 1] < 128;
            if (key_bytes[k] >= 128) continue;
            // skip class 03 / flex class 04 (classencoder.h:61-62): the orders' prune would erase skipgrams and flexgrams by their size too, and nothing here counts them
            if (first && (key_bytes[k] == 3 || key_bytes[k] == 4)) {
                (void)colibri_set_constraint(c, nullptr, nullptr, 0);
                return fail(c, COLIBRI_ERR_UNSUPPORTED, "seed set: skipgrams and flexgrams are not on the accelerated path (pattern %llu)", (unsigned long long)p);
            }
            ++ntok;
        }
        if (ntok == 0 || (key_off[p + 1] > key_off[p] && key_bytes[key_off[p + 1] - 1] >= 128)) {
            (void)colibri_set_constraint(c, nullptr, nullptr, 0);
            return fail(c, COLIBRI_ERR_ARG, "seed set: pattern %llu is empty or ends inside a token", (unsigned long long)p);
        }
        order[(size_t)p] = (uint8_t)std::min<uint32_t>(ntok, 255u);  // (orders from COLIBRI_MAX_ORDER on are never visited: such a seed simply stays)
        if (ntok < 128) orders[ntok >> 6] |= 1ull << (ntok & 63);
    }
    int rc = colibri_set_constraint(c, key_off, key_bytes, npatterns);  // the keys and their table; clears whatever set was installed
    if (rc || npatterns == 0) return rc;
    auto& cs = c->cs;
    cs.n     = 0;  // (until the rest is in place)
    if ((rc = dev_alloc(c, cs.seed_count, (size_t)npatterns)) || (rc = dev_alloc(c, cs.seed_slot, (size_t)npatterns)) || (rc = dev_alloc(c, cs.seed_row, (size_t)npatterns)) ||
        (rc = dev_alloc(c, cs.seed_order, (size_t)npatterns)) || (rc = dev_alloc(c, cs.seed_kept, (size_t)npatterns)) || (rc = dev_alloc(c, cs.seed_info, 1)))
        return rc;
    HIP_TRY(c, hipMemcpyAsync(cs.seed_count.p, counts, sizeof(uint32_t) * npatterns, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(cs.seed_order.p, order.data(), npatterns, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(cs.seed_info.p, 0, sizeof(SeedInfo), c->stream));
    hipLaunchKernelGGL(seed_closed_kernel, dim3(stream_grid(npatterns)), dim3(kBlock), 0, c->stream, cs.bytes.p, cs.off.p, (uint32_t)npatterns, cs.table.p, cs.cap, cs.seed_count.p, cs.seed_info.p);
    SeedInfo info{};
    info.open = 1;
    HIP_TRY(c, hipMemcpyAsync(&info, cs.seed_info.p, sizeof info, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    cs.seed_open = info.open != 0;
    cs.orders[0] = orders[0];
    cs.orders[1] = orders[1];
    cs.seed      = true;
    cs.seed_ran  = false;
    cs.n         = (uint32_t)npatterns;
    return COLIBRI_OK;
}

int colibri_seed_fetch(colibri_ctx* c, uint32_t* row_of_seed, uint8_t* kept) {
    if (!c || !row_of_seed || !kept) return COLIBRI_ERR_ARG;
    const auto& cs = c->cs;
    if (!cs.seed || cs.n == 0 || !cs.seed_ran || !c->trained) return fail(c, COLIBRI_ERR_STATE, "colibri_seed_fetch: no seeded colibri_train has run on the installed seed set");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(row_of_seed, cs.seed_row.p, sizeof(uint32_t) * cs.n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(kept, cs.seed_kept.p, cs.n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return COLIBRI_OK;
}
