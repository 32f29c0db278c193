// rsqc_group.cpp -- the exchange step of a sharded run: one context's result ranges summed into another's, by peer copy or by RCCL.
#include <rccl/rccl.h>   // types only: the library is bound at run time (rccl_api_ptr)
#include <dlfcn.h>
#include "rsqc_ctx.h"

int rsqc_reduce_peer(rsqc_ctx *dst, rsqc_ctx *src) {
    if (!dst || !src || dst == src || !dst->have_ann || !src->have_ann || !dst->finalized || !src->finalized) return RSQC_ERR_ARG;
    if (dst->arena_bytes != src->arena_bytes || dst->n_genes != src->n_genes || dst->n_exons != src->n_exons)
        return fail(dst, RSQC_ERR_ARG, "rsqc_reduce_peer: the two contexts hold different annotations");
    HIP_TRY(src, hipSetDevice(src->device));
    HIP_TRY(src, hipStreamSynchronize(src->stream));
    HIP_TRY(dst, hipSetDevice(dst->device));
    // the peer's three ranges are contiguous in its arena: [off_u64, off_ehit)
    const size_t lo = dst->off_u64, hi = dst->off_ehit, bytes = hi - lo;
    DevBuf tmp;
    int rc = dev_alloc(dst, tmp, bytes, false);
    if (rc) return rc;
    HIP_TRY(dst, hipMemcpyPeerAsync(tmp.p, dst->device, (const char *)src->d_arena.p + lo, src->device, bytes, dst->stream));
    char *D = (char *)dst->d_arena.p, *T = (char *)tmp.p - lo;
    launch_reduce_add(dst->stream, (unsigned long long *)(D + dst->off_u64), (const unsigned long long *)(T + dst->off_u64), (dst->off_exon - dst->off_u64) / 8,
                      (double *)(D + dst->off_exon), (const double *)(T + dst->off_exon), (dst->off_gvalid - dst->off_exon) / 8,
                      (uint8_t *)(D + dst->off_gvalid), (const uint8_t *)(T + dst->off_gvalid), dst->off_ehit - dst->off_gvalid);
    HIP_TRY(dst, hipGetLastError());
    HIP_TRY(dst, hipStreamSynchronize(dst->stream));
    tmp.release();
    // the device error flags travel too: a shard's failure is the run's failure
    int err = 0;
    HIP_TRY(src, hipSetDevice(src->device));
    HIP_TRY(src, hipMemcpy(&err, src->acc.error, sizeof(int), hipMemcpyDeviceToHost));
    if (err) { dst->sticky = err; return fail(dst, err, "a shard reported a device-side error"); }
    return RSQC_OK;
}

// ---- the exchange step of a sharded run as ONE RCCL reduction per result range (north_star: "an RCCL
// reduce of the per-gene count vectors and scalar metrics over xGMI at end-of-file") ---------------------------------------
// One process drives the node's GPUs (the command line with --gpus), so the communicators come from ncclCommInitAll over
// the contexts' devices and the three reductions of every GPU are issued inside one group call, each on its context's
// stream.  librccl is bound at run time (like libdeflate in the host reader): a machine without it, or two contexts on
// one device (a communicator cannot hold a device twice: the single-GPU test configuration RSQC_GPU_LIST=0,0), takes the
// peer-copy path below instead.
namespace {
struct RcclApi {
    void *lib = nullptr;
    ncclResult_t (*CommInitAll)(ncclComm_t *, int, const int *) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    ncclResult_t (*Reduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, int, ncclComm_t, hipStream_t) = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
    bool ok = false;
};
static RcclApi *rccl_api_ptr() {
    static RcclApi A;
    static bool tried = false;
    if (tried) return &A;
    tried = true;
    if (getenv("RSQC_NO_RCCL")) return &A;
    // the librccl that sits beside the HIP runtime THIS library runs on: a process may hold a second ROCm stack (PyTorch
    // bundles its own runtime and RCCL), and a communicator of that one cannot touch this runtime's allocations
    std::vector<std::string> names;
    Dl_info di{};
    if (dladdr(reinterpret_cast<const void *>(static_cast<hipError_t (*)(hipStream_t)>(&hipStreamSynchronize)), &di) && di.dli_fname) {
        std::string dir(di.dli_fname);
        const size_t slash = dir.find_last_of('/');
        if (slash != std::string::npos) { dir.resize(slash + 1); names.push_back(dir + "librccl.so.1"); names.push_back(dir + "librccl.so"); }
    }
    names.push_back("librccl.so.1"); names.push_back("librccl.so");
    for (const std::string &name : names) { A.lib = dlopen(name.c_str(), RTLD_NOW | RTLD_LOCAL); if (A.lib) break; }
    if (!A.lib) return &A;
#define RSQC_RCCL_SYM(field, sym) A.field = reinterpret_cast<decltype(A.field)>(dlsym(A.lib, sym))
    RSQC_RCCL_SYM(CommInitAll, "ncclCommInitAll"); RSQC_RCCL_SYM(CommDestroy, "ncclCommDestroy"); RSQC_RCCL_SYM(GroupStart, "ncclGroupStart");
    RSQC_RCCL_SYM(GroupEnd, "ncclGroupEnd"); RSQC_RCCL_SYM(Reduce, "ncclReduce"); RSQC_RCCL_SYM(GetErrorString, "ncclGetErrorString");
#undef RSQC_RCCL_SYM
    A.ok = A.CommInitAll && A.CommDestroy && A.GroupStart && A.GroupEnd && A.Reduce && A.GetErrorString;
    return &A;
}
}  // namespace

// A group = the contexts of one sharded run + (when RCCL is usable on their devices) one communicator per context, made
// ONCE: ncclCommInitAll over eight GPUs takes longer than the whole BAM loop of a 100 M-record file, so the command line
// brings the group up beside the GTF parse, outside the reference's `Average Reads/Sec` window (src/RNASeQC.cpp:385-394),
// and the end-of-file exchange only issues the reductions.
struct rsqc_group {
    std::vector<rsqc_ctx *> ctxs;
    std::vector<ncclComm_t> comms;       // empty: the peer-copy path
    std::string note;                    // why RCCL is not in use (for -vv)
    double init_ms = 0.0, last_reduce_ms = 0.0;
};

int rsqc_group_create(rsqc_ctx **ctxs, int n, rsqc_group **out) {
    if (!out) return RSQC_ERR_ARG;
    *out = nullptr;
    if (!ctxs || n < 1) return RSQC_ERR_ARG;
    for (int i = 0; i < n; ++i) if (!ctxs[i]) return RSQC_ERR_ARG;
    rsqc_group *g = new rsqc_group();
    g->ctxs.assign(ctxs, ctxs + n);
    const auto t0 = std::chrono::steady_clock::now();
    bool distinct = true;
    for (int i = 0; i < n; ++i) for (int j = 0; j < i; ++j) if (ctxs[i]->device == ctxs[j]->device) distinct = false;
    RcclApi &R = *rccl_api_ptr();
    if (!R.ok) g->note = getenv("RSQC_NO_RCCL") ? "RSQC_NO_RCCL is set" : "librccl not found";
    else if (!distinct) g->note = "two contexts share a device";
    else {
        std::vector<int> devs((size_t)n);
        for (int i = 0; i < n; ++i) devs[(size_t)i] = ctxs[i]->device;
        g->comms.assign((size_t)n, nullptr);
        const ncclResult_t r = R.CommInitAll(g->comms.data(), n, devs.data());
        if (r != ncclSuccess) {
            // no P2P / no shared memory / a mismatched RCCL: not an error of the run -- the peer-copy path sums the shards
            g->note = std::string("ncclCommInitAll: ") + R.GetErrorString(r);
            for (ncclComm_t c : g->comms) if (c) (void)R.CommDestroy(c);
            g->comms.clear();
        }
        (void)hipSetDevice(ctxs[0]->device);
    }
    g->init_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    *out = g;
    return RSQC_OK;
}

void rsqc_group_destroy(rsqc_group *g) {
    if (!g) return;
    if (!g->comms.empty()) { RcclApi &R = *rccl_api_ptr(); for (ncclComm_t c : g->comms) if (c) (void)R.CommDestroy(c); }
    delete g;
}

int rsqc_group_info(const rsqc_group *g, int *uses_rccl, double *init_ms, double *last_reduce_ms, const char **note) {
    if (!g) return RSQC_ERR_ARG;
    if (uses_rccl) *uses_rccl = g->comms.empty() ? 0 : 1;
    if (init_ms) *init_ms = g->init_ms;
    if (last_reduce_ms) *last_reduce_ms = g->last_reduce_ms;
    if (note) *note = g->note.c_str();
    return RSQC_OK;
}

static int shard_error_flags(rsqc_ctx *root, const std::vector<rsqc_ctx *> &ctxs) {
    for (size_t i = 1; i < ctxs.size(); ++i) {      // the device error flags travel too: a shard's failure is the run's failure
        int err = 0;
        HIP_TRY(ctxs[i], hipSetDevice(ctxs[i]->device));
        HIP_TRY(ctxs[i], hipMemcpy(&err, ctxs[i]->acc.error, sizeof(int), hipMemcpyDeviceToHost));
        if (err) { root->sticky = err; return fail(root, err, "a shard reported a device-side error"); }
    }
    HIP_TRY(root, hipSetDevice(root->device));
    return RSQC_OK;
}

int rsqc_group_reduce(rsqc_group *g, int *used_rccl) {
    if (used_rccl) *used_rccl = 0;
    if (!g || g->ctxs.empty()) return RSQC_ERR_ARG;
    const int n = (int)g->ctxs.size();
    rsqc_ctx *root = g->ctxs[0];
    for (int i = 0; i < n; ++i) {
        rsqc_ctx *c = g->ctxs[(size_t)i];
        if (!c->have_ann || !c->finalized) return RSQC_ERR_ARG;
        if (c->arena_bytes != root->arena_bytes || c->n_genes != root->n_genes || c->n_exons != root->n_exons)
            return fail(root, RSQC_ERR_ARG, "rsqc_group_reduce: the contexts hold different annotations");
    }
    const auto t0 = std::chrono::steady_clock::now();
    auto done = [&](int rc) { g->last_reduce_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); return rc; };
    if (!g->comms.empty()) {
        RcclApi &R = *rccl_api_ptr();
        // the three reducible ranges of the arena (rsqc_device_vectors): u64 counts | f64 sums + owner-only statistics | u8 flags
        const size_t n_u64 = (root->off_exon - root->off_u64) / 8, n_f64 = (root->off_gvalid - root->off_exon) / 8, n_u8 = root->off_ehit - root->off_gvalid;
        ncclResult_t r = R.GroupStart();
        bool issued = false;
        if (r == ncclSuccess) {
            for (int i = 0; i < n && r == ncclSuccess; ++i) {
                rsqc_ctx *c = g->ctxs[(size_t)i];
                char *A = (char *)c->d_arena.p;
                (void)hipSetDevice(c->device);
                r = R.Reduce(A + c->off_u64, A + c->off_u64, n_u64, ncclUint64, ncclSum, 0, g->comms[(size_t)i], c->stream);
                if (r == ncclSuccess) r = R.Reduce(A + c->off_exon, A + c->off_exon, n_f64, ncclFloat64, ncclSum, 0, g->comms[(size_t)i], c->stream);
                if (r == ncclSuccess) r = R.Reduce(A + c->off_gvalid, A + c->off_gvalid, n_u8, ncclUint8, ncclSum, 0, g->comms[(size_t)i], c->stream);
                issued = true;
            }
            const ncclResult_t re = R.GroupEnd();
            if (r == ncclSuccess) r = re;
        }
        if (r != ncclSuccess) {
            // a reduction that was (partly) enqueued may have changed ctxs[0]'s ranges, and waiting on a half-issued group can
            // hang: nothing is synchronised, the run ends here.  A failure before anything was issued takes the peer path.
            if (issued) return done(fail(root, RSQC_ERR_HIP, std::string("RCCL reduction failed after it was issued: ") + R.GetErrorString(r)));
            g->note = std::string("ncclGroupStart: ") + R.GetErrorString(r);
        } else {
            for (int i = 0; i < n; ++i) {
                rsqc_ctx *c = g->ctxs[(size_t)i];
                (void)hipSetDevice(c->device);
                if (hipStreamSynchronize(c->stream) != hipSuccess) return done(fail(root, RSQC_ERR_HIP, "hipStreamSynchronize after the RCCL reduction failed"));
            }
            const int rc = shard_error_flags(root, g->ctxs);
            if (rc == RSQC_OK && used_rccl) *used_rccl = 1;
            return done(rc);
        }
    }
    for (int i = 1; i < n; ++i) { const int rc = rsqc_reduce_peer(root, g->ctxs[(size_t)i]); if (rc != RSQC_OK) return done(rc); }
    return done(RSQC_OK);
}

// create + reduce + destroy in one call (a caller that does not mind the bring-up inside its timed region)
int rsqc_reduce_group(rsqc_ctx **ctxs, int n, int *used_rccl) {
    if (used_rccl) *used_rccl = 0;
    rsqc_group *g = nullptr;
    int rc = rsqc_group_create(ctxs, n, &g);
    if (rc != RSQC_OK) return rc;
    rc = rsqc_group_reduce(g, used_rccl);
    rsqc_group_destroy(g);
    return rc;
}
