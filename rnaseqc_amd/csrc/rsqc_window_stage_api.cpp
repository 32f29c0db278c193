// rsqc_window_stage_api.cpp -- what rsqc_cycle_api.cpp, rsqc_mismatch_api.cpp and rsqc_allele_api.cpp have in common: a stage that hangs
// one kernel behind every window of the device decode and counts into device-resident tables.  Its begin (the order of the calls, the
// tables reserved and cleared), the kernel of a window between a pair of events, what the host adds, and its end (one read-back a pass,
// never a partial table).  The public calls' names and the stage's noun are parameters; the list of the stages is here and nowhere else.
#include <array>

#include "rsqc_ctx.h"

namespace rsqc {

namespace {

struct Listed {
    WindowStage &st;
    void (*launch)(rsqc_ctx *, const DecodeWindow &, const SamWindow *);
    void (*drop)(rsqc_ctx *, bool);
    bool has_inputs;               // a packed reference, a site list: freed with the context's inputs
};
// in the order of their kernels behind a window
std::array<Listed, 3> stages(rsqc_ctx *c) {
    return {{{c->cyc, cycle_launch, cycle_drop, false}, {c->mm, mismatch_launch, mismatch_drop, true}, {c->al, alleles_launch, alleles_drop, true}}};
}

void recycle_events(rsqc_ctx *c, WindowStage &S) {
    for (auto &pr : S.events) { c->event_pool.push_back(pr.first); c->event_pool.push_back(pr.second); }
    S.events.clear();
}

int end_run(rsqc_ctx *c, WindowStage &S, size_t bytes, int (*finish)(rsqc_ctx *, double)) {
    HIP_TRY(c, hipMemcpyAsync(S.h_tab.p, S.tab.p, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    double total = 0;
    for (auto &pr : S.events) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) total += ms;
    }
    recycle_events(c, S);
    return finish(c, total);
}

}  // namespace

void window_stages_seen(rsqc_ctx *c, uint64_t n_rec) {
    for (const Listed &L : stages(c)) if (L.st.active) L.st.seen += n_rec;
}

int window_stages_launch(rsqc_ctx *c, const DecodeWindow &W, const SamWindow *S) {
    for (const Listed &L : stages(c)) {
        if (!L.st.active) continue;
        hipEvent_t e0 = get_event(c), e1 = get_event(c);
        L.st.events.emplace_back(e0, e1);
        HIP_TRY(c, hipEventRecord(e0, c->stream));
        L.launch(c, W, S);
        HIP_TRY(c, hipEventRecord(e1, c->stream));
    }
    return 0;
}

void window_stages_drop(rsqc_ctx *c, bool free_tables, bool free_inputs) {
    for (const Listed &L : stages(c)) L.drop(c, free_tables || (free_inputs && L.has_inputs));
}

int window_begin_check(rsqc_ctx *c, const WindowStage &S, const WindowNames &N) {
    if (c->sticky) return c->sticky;
    if (c->finalized) return fail(c, RSQC_ERR_ARG, "rsqc_reset required after rsqc_finalize");
    if (S.active) return fail(c, RSQC_ERR_ARG, std::string(N.begin) + ": the context is counting " + N.noun + " already");
    if (c->dec.active || c->name_mode >= 0 || !c->batch_file_index.empty() || c->next_record_base)
        return fail(c, RSQC_ERR_ARG, std::string(N.begin) + " must precede the first submit and the rsqc_decode_begin of the pass");
    return 0;
}

int window_tables(rsqc_ctx *c, WindowStage &S, size_t bytes, const std::string &no_device, const std::string &no_host) {
    if (!dev_reserve(S.tab, bytes)) return fail(c, RSQC_ERR_CAPACITY, no_device);
    if (!host_reserve(S.h_tab, bytes)) return fail(c, RSQC_ERR_CAPACITY, no_host);
    HIP_TRY(c, hipMemsetAsync(S.tab.p, 0, bytes, c->stream));
    return 0;
}

// (the words the host added go back to the allocator: with --alleles they can be over a gigabyte, with the other two the cost is nothing;
// a stage's info is filled anew by its `finish` before an end hands it out, so a drop leaves it)
void window_drop(rsqc_ctx *c, WindowStage &S, bool free_tables) {
    recycle_events(c, S);
    S.active = S.done = false;
    S.seen = S.added_seen = 0;
    S.added.clear(); S.added.shrink_to_fit();
    if (free_tables) { S.tab.release(); S.h_tab.release(); }
}

int window_add_check(rsqc_ctx *c, const WindowStage &S, const WindowNames &N) {
    if (c->sticky) return c->sticky;
    if (!S.active) return fail(c, RSQC_ERR_ARG, std::string(N.begin) + " must precede " + N.add);
    if (S.done) return fail(c, RSQC_ERR_ARG, std::string(N.add) + " behind " + N.end);
    return 0;
}

uint64_t *window_added(WindowStage &S, size_t words) {
    if (S.added.empty()) S.added.assign(words, 0);
    return S.added.data();
}

int window_end(rsqc_ctx *c, WindowStage &S, const WindowNames &N, size_t bytes, int (*finish)(rsqc_ctx *, double)) {
    if (c->sticky) return c->sticky;
    if (!S.active) return fail(c, RSQC_ERR_ARG, std::string(N.begin) + " must precede " + N.end);
    if (c->dec.active) return fail(c, RSQC_ERR_ARG, std::string("rsqc_decode_end must precede ") + N.end);
    if (!S.done) {
        HIP_TRY(c, hipSetDevice(c->device));
        const int rc = end_run(c, S, bytes, finish);
        if (rc) { (void)hipStreamSynchronize(c->stream); c->sticky = rc; return rc; }       // never a partial table: the pass is void until rsqc_reset
        S.done = true;
    }
    return 0;
}

void window_sum_added(const WindowStage &S, uint64_t *h, size_t words) {
    if (!S.added.empty()) for (size_t k = 0; k < words; ++k) h[k] += S.added[k];
}

}  // namespace rsqc
