// sbm_capi_multi.inc — part of libsbm_hip.so's host side (included by sbm_capi.hip, one translation unit): multi-GPU entry points -- RCCL (resolved with dlopen), template-sharded and build-sharded steps, single-process multi-context match.

// ---- RCCL exchange step (resolved at run time: the library itself does not link librccl) ----
namespace {
struct Id128 { // ncclUniqueId is passed by value
    char b[128];
};
struct Rccl {
    void* h = nullptr;
    int (*GetUniqueId)(void*) = nullptr;
    int (*CommInitRank)(void**, int, Id128, int) = nullptr;
    int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    int (*CommCount)(void*, int*) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
};
Rccl g_rccl;
int rccl_load()
{
    if (g_rccl.h) return 0;
    const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (const char* n : names)
        if ((g_rccl.h = dlopen(n, RTLD_NOW | RTLD_GLOBAL))) break;
    if (!g_rccl.h) return fail(SBM_ERR_HIP, "cannot load librccl: %s", dlerror());
    g_rccl.GetUniqueId = (decltype(g_rccl.GetUniqueId))dlsym(g_rccl.h, "ncclGetUniqueId");
    g_rccl.CommInitRank = (decltype(g_rccl.CommInitRank))dlsym(g_rccl.h, "ncclCommInitRank");
    g_rccl.AllGather = (decltype(g_rccl.AllGather))dlsym(g_rccl.h, "ncclAllGather");
    g_rccl.CommDestroy = (decltype(g_rccl.CommDestroy))dlsym(g_rccl.h, "ncclCommDestroy");
    g_rccl.GetErrorString = (decltype(g_rccl.GetErrorString))dlsym(g_rccl.h, "ncclGetErrorString");
    g_rccl.GroupStart = (decltype(g_rccl.GroupStart))dlsym(g_rccl.h, "ncclGroupStart");
    g_rccl.GroupEnd = (decltype(g_rccl.GroupEnd))dlsym(g_rccl.h, "ncclGroupEnd");
    g_rccl.CommCount = (decltype(g_rccl.CommCount))dlsym(g_rccl.h, "ncclCommCount");
    g_rccl_destroy_hook = [](sbm_ctx* c) {
        if (c->comm) g_rccl.CommDestroy(c->comm);
        c->comm = nullptr;
    };
    if (!g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.AllGather || !g_rccl.CommDestroy || !g_rccl.GroupStart || !g_rccl.GroupEnd) {
        g_rccl.h = nullptr;
        return fail(SBM_ERR_HIP, "librccl lacks the expected entry points");
    }
    return 0;
}
const char* rccl_err(int rc) { return g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "nccl error"; }
} // namespace

extern "C" int sbm_comm_unique_id(void* id_out)
{
    if (!id_out) return fail(SBM_ERR_INVALID, "null argument");
    if (int e = rccl_load()) return e;
    int rc = g_rccl.GetUniqueId(id_out);
    if (rc) return fail(SBM_ERR_HIP, "ncclGetUniqueId: %s", rccl_err(rc));
    return 0;
}

extern "C" int sbm_comm_init(sbm_ctx* c, int32_t world, int32_t rank, const void* id)
{
    if (!c || !id || world < 1 || rank < 0 || rank >= world) return fail(SBM_ERR_INVALID, "bad communicator arguments");
    if (int e = rccl_load()) return e;
    HIP_TRY(hipSetDevice(c->cfg.device_id));
    if (c->comm) {
        g_rccl.CommDestroy(c->comm);
        c->comm = nullptr;
    }
    Id128 uid;
    memcpy(uid.b, id, 128);
    int rc = g_rccl.CommInitRank(&c->comm, world, uid, rank);
    if (rc) return fail(SBM_ERR_HIP, "ncclCommInitRank: %s", rccl_err(rc));
    c->comm_world = world;
    c->comm_rank = rank;
    return 0;
}

extern "C" int sbm_comm_destroy(sbm_ctx* c)
{
    if (!c) return fail(SBM_ERR_INVALID, "null context");
    if (c->comm && g_rccl.CommDestroy) {
        (void)hipDeviceSynchronize();
        g_rccl.CommDestroy(c->comm);
    }
    c->comm = nullptr;
    c->comm_world = 0;
    return 0;
}

extern "C" int sbm_comm_count(sbm_ctx* c, int32_t* n_ranks)
{
    if (!c || !n_ranks) return fail(SBM_ERR_INVALID, "null argument");
    if (!c->comm) return fail(SBM_ERR_STATE, "sbm_comm_init has not been called on this context");
    if (!g_rccl.CommCount) return fail(SBM_ERR_HIP, "librccl lacks ncclCommCount");
    int n = 0;
    int rc = g_rccl.CommCount(c->comm, &n);
    if (rc) return fail(SBM_ERR_HIP, "ncclCommCount: %s", rccl_err(rc));
    *n_ranks = n;
    return 0;
}

// the exchange step every sharded entry point ends with: every rank's shard to every rank (ncclAllGather over xGMI on the
// kernels' stream; without a communicator the local shard is all there is), optionally copied on into device-visible host memory
static int gather_shards(sbm_ctx* c, hipStream_t s, const void* d_local, size_t bytes, void* d_gathered, void* gathered_mirror)
{
    const void* result = d_local;
    size_t total = bytes;
    if (c->comm) {
        int rc = g_rccl.AllGather(d_local, d_gathered, bytes, /* ncclUint8 */ 1, c->comm, s);
        if (rc) return fail(SBM_ERR_HIP, "ncclAllGather: %s", rccl_err(rc));
        result = d_gathered;
        total = bytes * (size_t)c->comm_world;
    }
    if (gathered_mirror) {
        hipLaunchKernelGGL(k_copy_bytes, dim3((unsigned)std::min<size_t>((total / 16 + 255) / 256 + 1, 1024)), dim3(256), 0, s,
                           (const uint8_t*)result, (uint8_t*)gathered_mirror, total);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

extern "C" int sbm_match_templates_device_sharded(sbm_ctx* c, float threshold, void* d_local, int64_t cap, void* d_gathered,
                                                  void* gathered_mirror, void* stream)
{
    if (!c || !d_local || !d_gathered) return fail(SBM_ERR_INVALID, "null argument");
    if (!c->comm) return fail(SBM_ERR_STATE, "sbm_comm_init has not been called on this context");
    const size_t bytes = (size_t)SBM_SHARD_HEADER_BYTES + (size_t)cap * sizeof(sbm_match_rec);
    if (int e = sbm_match_templates_device(c, threshold, (char*)d_local + SBM_SHARD_HEADER_BYTES, cap, d_local, stream)) return e;
    return gather_shards(c, launch_stream(c, stream), d_local, bytes, d_gathered, gathered_mirror);
}

extern "C" int sbm_match_device_sharded(sbm_ctx* c, const void* d_img, int32_t rows, int32_t cols, int32_t stride, int32_t channels,
                                        const void* d_mask, float threshold, void* d_local, int64_t cap, void* d_gathered,
                                        void* gathered_mirror, void* stream)
{
    if (!c || !d_local || !d_gathered) return fail(SBM_ERR_INVALID, "null argument");
    if (!c->comm) return fail(SBM_ERR_STATE, "sbm_comm_init has not been called on this context");
    const size_t bytes = (size_t)SBM_SHARD_HEADER_BYTES + (size_t)cap * sizeof(sbm_match_rec);
    // this rank's shard: {n_matches, overflow, 0, 0} header followed by the records
    if (int e = sbm_match_device(c, d_img, rows, cols, stride, channels, d_mask, threshold, (char*)d_local + SBM_SHARD_HEADER_BYTES, cap,
                                 d_local, stream))
        return e;
    // the one exchange step of the path: every rank's list to every rank, over xGMI, on the same stream
    return gather_shards(c, launch_stream(c, stream), d_local, bytes, d_gathered, gathered_mirror);
}

extern "C" int sbm_match_batch_device_sharded(sbm_ctx* c, const void* d_imgs, int64_t frame_stride, int32_t n_frames, int32_t rows,
                                              int32_t cols, int32_t stride, int32_t channels, const void* d_mask, float threshold,
                                              void* d_local, int64_t cap, void* d_gathered, void* gathered_mirror, void* stream)
{
    if (!c || !d_local || !d_gathered) return fail(SBM_ERR_INVALID, "null argument");
    if (!c->comm) return fail(SBM_ERR_STATE, "sbm_comm_init has not been called on this context");
    if (n_frames < 1) return fail(SBM_ERR_INVALID, "n_frames must be >= 1");
    // this rank's shard: n_frames {n_matches, overflow} pairs (padded to 16 bytes), then n_frames blocks of cap records
    const size_t header = ((size_t)n_frames * 8 + 15) / 16 * 16;
    const size_t bytes = header + (size_t)n_frames * (size_t)cap * sizeof(sbm_match_rec);
    if (int e = sbm_match_batch_device(c, d_imgs, frame_stride, n_frames, rows, cols, stride, channels, d_mask, threshold,
                                       (char*)d_local + header, cap, d_local, stream))
        return e;
    return gather_shards(c, launch_stream(c, stream), d_local, bytes, d_gathered, gathered_mirror);
}

// the exchange of the build-sharded step: every rank's row band of every level's orientation map, in place
// (rank r's band of frame f already sits at its final address: ncclAllGather with sendbuff = recvbuff + r * count),
// all frames and levels in one ncclGroup = one fused launch on the kernels' stream
static int gather_bands(sbm_ctx* c, hipStream_t s, int frames)
{
    int rc = g_rccl.GroupStart();
    if (rc) return fail(SBM_ERR_HIP, "ncclGroupStart: %s", rccl_err(rc));
    for (int l = 0; l < c->L && !rc; ++l) {
        const size_t fs = (size_t)c->rows[l] * c->cols[l], cnt = fs / (size_t)c->comm_world;
        for (int f = 0; f < frames && !rc; ++f) {
            uint8_t* recv = c->d_quant[l].as<uint8_t>() + (size_t)f * fs;
            rc = g_rccl.AllGather(recv + (size_t)c->comm_rank * cnt, recv, cnt, /* ncclUint8 */ 1, c->comm, s);
        }
    }
    const int rc2 = g_rccl.GroupEnd();
    if (rc || rc2) return fail(SBM_ERR_HIP, "ncclAllGather (bands): %s", rccl_err(rc ? rc : rc2));
    return 0;
}

extern "C" int sbm_match_batch_device_banded(sbm_ctx* c, const void* d_imgs, int64_t frame_stride, int32_t n_frames, int32_t rows,
                                             int32_t cols, int32_t stride, int32_t channels, const void* d_mask, float threshold,
                                             void* d_local, int64_t cap, void* d_gathered, void* gathered_mirror, int32_t n_bands,
                                             void* stream)
{
    if (!c || !d_local) return fail(SBM_ERR_INVALID, "null argument");
    MatchCall m{strided_frames(d_imgs, stride, channels, n_frames, frame_stride), strided_masks(d_mask, 0), rows, cols, threshold,
                (sbm_match_rec*)d_local, cap, (int32_t*)d_local};
    if (int e = check_match_call(c, m)) return e;
    // this rank's shard, as sbm_match_batch_device_sharded lays it out: the records follow the header of counts
    const size_t header = ((size_t)n_frames * 8 + 15) / 16 * 16;
    const size_t bytes = header + (size_t)n_frames * (size_t)cap * sizeof(sbm_match_rec);
    m.out = (sbm_match_rec*)((char*)d_local + header);
    const bool comm = c->comm != nullptr;
    if (comm && !d_gathered) return fail(SBM_ERR_INVALID, "d_gathered is required with a communicator");
    const bool multi = comm && c->comm_world > 1;
    if (multi && n_bands != 0 && n_bands != c->comm_world)
        return fail(SBM_ERR_INVALID, "n_bands %d != communicator size %d", n_bands, c->comm_world);
    if (multi) n_bands = c->comm_world;
    if (n_bands < 1) return fail(SBM_ERR_INVALID, "n_bands must be >= 1 on a single GPU");
    Bands b;
    b.n = n_bands;
    b.first = multi ? c->comm_rank : 0;  // several ranks: this rank's band, then the exchange
    b.count = multi ? 1 : n_bands;       // one GPU: every band, one launch each (rehearsal of the band launches; with a
    b.between = comm ? gather_bands : nullptr; // one-rank communicator also of the grouped in-place all-gathers)
    hipStream_t s;
    if (int e = begin_match(c, stream, m, &s, &b)) return e;
    // a result mirror set on the context would be written by the last kernel; the gathered mirror below replaces it
    if (int e = enqueue_match(c, s, m, &b)) return e;
    call_enqueued(c, s);
    // the second exchange of the step: the per-rank match lists
    return gather_shards(c, s, d_local, bytes, d_gathered, gathered_mirror);
}

// Single-process multi-GPU match (SURVEY.md 8b: sbm_match_sharded(ctxs[], n_gpus, ...)): the analogue of the reference's
// OpenMP team (line2Dup.cpp:1166-1170) with one host thread and one context per GPU.  Every context holds the same
// templates and its own selection (sbm_partition_templates + sbm_select_range / sbm_select_templates); the frame goes to
// every GPU, each matches its template shard, the lists are concatenated on the host (the reduction of :1168).
extern "C" int sbm_match_sharded(sbm_ctx* const* ctxs, int32_t n_ctx, const uint8_t* img, int32_t rows, int32_t cols, int32_t stride,
                                 int32_t channels, const uint8_t* mask, float threshold, sbm_match_rec* out, int64_t cap, int64_t* n_out)
{
    if (!ctxs || n_ctx < 1 || !n_out || (!out && cap > 0)) return fail(SBM_ERR_INVALID, "bad arguments");
    for (int i = 0; i < n_ctx; ++i)
        if (!ctxs[i]) return fail(SBM_ERR_INVALID, "context %d is null", i);
    if (n_ctx == 1) return sbm_match(ctxs[0], img, rows, cols, stride, channels, mask, threshold, out, cap, n_out);
    struct Shard {
        std::vector<sbm_match_rec> recs;
        int64_t n = 0;
        int rc = 0;
        std::string err;
    };
    std::vector<Shard> sh(n_ctx);
    std::vector<std::thread> th;
    for (int i = 0; i < n_ctx; ++i)
        th.emplace_back([&, i]() {
            Shard& me = sh[i];
            me.recs.resize((size_t)std::max<int64_t>(cap, 1));
            me.rc = sbm_match(ctxs[i], img, rows, cols, stride, channels, mask, threshold, me.recs.data(), (int64_t)me.recs.size(), &me.n);
            if (me.rc) me.err = sbm_last_error(); // the message is thread-local: carry it to the caller's thread
        });
    for (auto& t : th) t.join();
    int64_t total = 0;
    for (int i = 0; i < n_ctx; ++i) {
        if (sh[i].rc && sh[i].rc != SBM_ERR_CAPACITY) return fail(sh[i].rc, "shard %d: %s", i, sh[i].err.c_str());
        total += sh[i].n;
    }
    *n_out = total;
    for (int i = 0; i < n_ctx; ++i)
        if (sh[i].rc == SBM_ERR_CAPACITY) return fail(SBM_ERR_CAPACITY, "shard %d: %s", i, sh[i].err.c_str());
    if (total > cap) return fail(SBM_ERR_CAPACITY, "%lld matches exceed the output capacity %lld", (long long)total, (long long)cap);
    int64_t k = 0;
    for (int i = 0; i < n_ctx; ++i) {
        if (sh[i].n > 0) memcpy(out + k, sh[i].recs.data(), (size_t)sh[i].n * sizeof(sbm_match_rec));
        k += sh[i].n;
    }
    return 0;
}

extern "C" {

int sbm_coarse_bytes(sbm_ctx* c, int64_t* bytes)
{
    if (!c || !bytes) return fail(SBM_ERR_INVALID, "null argument");
    if (c->rec.levels_valid < c->L) return fail(SBM_ERR_STATE, "pyramid not built");
    if (int e = ensure_host_fxy(c)) return e; // (a device install leaves the features on the device)
    const int lc = c->L - 1, T = c->cfg.T[lc], W = c->cols[lc] / T, H = c->rows[lc] / T;
    int64_t total = 0;
    for (int32_t t : c->h_active) {
        const DevTL& tl = c->h_tls[(size_t)t * c->L + lc];
        const int npos = host_template_npos(tl, T, W, H);
        if (npos > 0) total += npos * features_in_bounds(c, tl, c->rows[lc], c->cols[lc]);
    }
    *bytes = total;
    return 0;
}

} // extern "C"

