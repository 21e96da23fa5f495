// sbm_capi_ctx.inc — part of libsbm_hip.so's host side (included by sbm_capi.hip, one translation unit): error handling, device buffers, the context (sbm_ctx) and the launch helpers every entry point uses (gradient stage, linear memories, coarse pass, refinement, graph capture).
namespace {

thread_local std::string g_err;
void (*g_rccl_destroy_hook)(sbm_ctx*) = nullptr; // set once librccl is loaded

int fail(int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(SBM_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// grow-only device buffer; frees itself, and cannot be copied
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    int ensure(size_t bytes, bool zero = false)
    {
        if (bytes <= cap && p) return 0;
        release();
        size_t want = bytes ? bytes : 16;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) return fail(SBM_ERR_HIP, "hipMalloc(%zu) failed: %s", want, hipGetErrorString(e));
        cap = want;
        if (zero) {
            // hipMemset of device memory is asynchronous to the host and runs on the null stream, which the engine's
            // (non-blocking) streams do not wait for: make the zeros land before anything can be enqueued behind them
            e = hipMemset(p, 0, want);
            if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
            if (e != hipSuccess) return fail(SBM_ERR_HIP, "hipMemset failed: %s", hipGetErrorString(e));
        }
        return 0;
    }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    void swap(DevBuf& o)
    {
        std::swap(p, o.p);
        std::swap(cap, o.cap);
    }
    template <class T>
    T* as() const { return (T*)p; }
};

struct Timing {
    const char* name;
    hipEvent_t a, b;
    bool shared_a = false; // a is the previous entry's b
};

int64_t lm_stride_for(int rows, int cols, int T)
{
    int64_t W = cols / T, H = rows / T;
    int64_t s = (int64_t)T * T * W * H + W * H + 16 * W + 80;
    return (s + 63) / 64 * 64;
}

} // namespace

// The A/B knobs of the builder's measurements (DESIGN.md sections 5, 6, 9): environment variables read ONCE per process,
// here and nowhere else; none is needed for correctness, results are identical under every setting.
//   SBM_COARSE=block|wave|bits|bytes   coarse-pass kernel (default: the bit-plane kernel whenever the threshold is >= 0;
//                             bytes: the round-3 choice between block and wave by launch size)
//   SBM_QUANTIZE=tile|stream  gradient kernel (default: by launch size; sbm_set_quantize_mode overrides per context)
//   SBM_QS_HS=a[,b]           rows per work item of the streaming gradient kernel (>= 1 Mpixel levels, smaller levels)
//   SBM_QS_PACK=0             no shared wave for the narrow last strip of several frames
//   SBM_FULL_LM=1             eight response planes at every level (no compact spread plane)
//   SBM_STRIP_LM=0            compact plane row-major instead of strip-interleaved
//   SBM_LOCAL_GRID=n          candidate slots per frame of the refinement pass
//   SBM_LOCAL_WAVES=4|16      waves per candidate of the refinement pass
//   SBM_LOCAL_ORDER=0|2       candidate-to-workgroup order of the refinement pass (default: by the batch's plane size)
//   SBM_GRAPH_FORK=0          single-frame hipGraph without the side branch
//   SBM_BITS_WIDE=0|1         bit-plane coarse pass: 8 features per batch throughout | 16 after the first 16 (default: 16 from 64
//                             features per template on -- c3, 31 features: 18.2 against 21.4 us; case1, 71: 26.2 against 24.9;
//                             c4, 4095: 4.30 against 4.04 ms, tools/r04_coarse_tune.sh)
//   SBM_MATCH_BANDS=n         sbm_match: the frame's upload in n row bands with level 0's gradient launches following band by band
//                             (default 0 = one copy: measured on ROCm 7.2, every band costs 16 - 30 us of copy + cross-stream event
//                             overhead -- Detector::match 115 us with one copy, 141 / 177 / 247 with 2 / 4 / 8 bands, tools/r04_latency.sh)
//   SBM_BITS_BLOCK=0|1        bit-plane coarse pass: never | always the eight-waves-per-item latency form (default: launches of <= 2048 items)
//   SBM_BITS_DW=1|2           bit-plane coarse pass: 32 | 64 positions per lane (default: 64 when the launch would need two rounds of waves)
//   SBM_LM_ALLTY=0            strip plane of a T = 4 level: a thread per (ty, gy) pixel row (round 2) instead of per grid row
//   SBM_FUSED_BITS=0          match entry points build the coarsest level's 8 response planes and pack the bit planes from them
//   SBM_LOCAL_BITS=0|1        refinement pass of a T = 4 strip level on spread bytes | on bit strips (sbm_local_bits.h;
//                             sbm_set_refine_bits overrides per context)
//   SBM_SPARSE_STRIPS=0       match entry points build level 0's bit strips whole, inside the one linear-memory launch, instead of
//                             only in the tiles the coarse candidates' refinement reads (sbm_refine_tiles.h)
//   SBM_SPARSE_GRADIENT=0     match entry points run level 0's whole gradient stage in front of the coarse pass instead of the source
//                             pass there (cv::pyrDown + retained copy) and the gradient of the flagged tiles' reach behind it
//                             (sbm_quantize_stream.h, QS_SOURCE / QS_SPARSE); SBM_SPARSE_STRIPS=0 implies it
//   SBM_SPARSE_RECTS=0        the sparse level-0 gradient pass takes its work items from the tile flags on the fixed strip grid instead of
//                             from the record of need rectangles (sbm_refine_tiles.h: refine_need, gradient_rect_item_needed): the A/B knob
//   SBM_SPARSE_LIST=0         the sparse level-0 gradient launch as one wave per item of its grid, every wave testing its own item, instead
//                             of SBM_SPARSE_SLOTS waves per frame that run from the lists of working items k_mark_refine_tiles leaves
//                             (sbm_refine_tiles.h: gradient_rect_list); nothing is allocated for the lists.  SBM_SPARSE_RECTS=0 implies it
//   SBM_SPARSE_SLOTS=n        waves per frame of that launch (default and at most: the items per frame)
//   SBM_SPARSE_LIST_HS=n      rows per item of the grid the lists are made on (default: sparse_list_plan's rule); 0: the launch's own
//                             grid, so that a listed frame's items are those the launch would test itself -- the A/B knob
//   SBM_QS_SRC_HS=n           rows per work item of the source pass (default 32: 35 row iterations in six groups of 6)
//   SBM_SOURCE_LINES=0        the source pass always in its strided form (QS_SOURCE), never as k_source_lines (sbm_source_lines.h), which
//                             otherwise runs wherever the caller's layout admits it (source_lines_ok): the A/B knob of the two forms
//   SBM_RETAIN_ALWAYS=1       every call of the sparse level-0 path stores the retained copy of its source and runs its sparse gradient
//                             launch on that copy, instead of storing it only while no later call is enqueued behind it and reading
//                             the caller's frames (DESIGN.md section 5): the A/B knob
struct Tuning {
    int coarse = 0, quantize = 0, hs0 = 0, hs1 = 0, local_grid = 0, local_waves = 0, local_order = -1;
    bool qs_pack = true, full_lm = false, strip_lm = true, graph_fork = true, fused_bits = true, lm_allty = true;
    int bits_wide = -1, bits_dw = 0, bits_block = -1, match_bands = 0, local_bits = -1;
    bool sparse_strips = true, sparse_gradient = true, source_lines = true, sparse_rects = true;
    int src_hs = 0;
    bool sparse_list = true;
    int sparse_slots = 0;
    int sparse_list_hs = -1;
    bool retain_always = false;
};
static const Tuning& tuning()
{
    static const Tuning t = [] {
        Tuning k;
        auto num = [](const char* name, int dflt) {
            const char* v = getenv(name);
            return v && *v ? atoi(v) : dflt;
        };
        if (const char* e = getenv("SBM_COARSE"))
            k.coarse = !strcmp(e, "block") ? 1 : (!strcmp(e, "wave") ? 2 : (!strcmp(e, "bits") ? 3 : (!strcmp(e, "bytes") ? 4 : 0)));
        if (const char* e = getenv("SBM_QUANTIZE")) k.quantize = !strcmp(e, "tile") ? 1 : (!strcmp(e, "stream") ? 2 : 0);
        if (const char* e = getenv("SBM_QS_HS")) {
            k.hs0 = atoi(e);
            k.hs1 = strchr(e, ',') ? atoi(strchr(e, ',') + 1) : k.hs0;
        }
        k.qs_pack = num("SBM_QS_PACK", 1) != 0;
        k.full_lm = num("SBM_FULL_LM", 0) != 0;
        k.strip_lm = num("SBM_STRIP_LM", 1) != 0;
        k.local_grid = std::max(0, num("SBM_LOCAL_GRID", 0));
        k.local_waves = num("SBM_LOCAL_WAVES", 0);
        k.local_order = num("SBM_LOCAL_ORDER", -1) == 2 ? 2 : num("SBM_LOCAL_ORDER", -1) == 0 ? 0 : -1;
        k.graph_fork = num("SBM_GRAPH_FORK", 1) != 0;
        k.fused_bits = num("SBM_FUSED_BITS", 1) != 0;
        k.bits_wide = num("SBM_BITS_WIDE", -1);
        k.lm_allty = num("SBM_LM_ALLTY", 1) != 0;
        k.bits_block = num("SBM_BITS_BLOCK", -1);
        k.local_bits = num("SBM_LOCAL_BITS", -1);
        k.sparse_strips = num("SBM_SPARSE_STRIPS", 1) != 0;
        k.sparse_gradient = k.sparse_strips && num("SBM_SPARSE_GRADIENT", 1) != 0;
        k.sparse_rects = k.sparse_gradient && num("SBM_SPARSE_RECTS", 1) != 0;
        k.sparse_list = k.sparse_rects && num("SBM_SPARSE_LIST", 1) != 0;
        k.sparse_slots = std::max(0, num("SBM_SPARSE_SLOTS", 0));
        k.sparse_list_hs = std::min(4096, std::max(-1, num("SBM_SPARSE_LIST_HS", -1)));
        k.src_hs = std::min(4096, std::max(0, num("SBM_QS_SRC_HS", 0)));
        k.source_lines = num("SBM_SOURCE_LINES", 1) != 0;
        k.retain_always = num("SBM_RETAIN_ALWAYS", 0) != 0;
        k.match_bands = std::min(8, std::max(0, num("SBM_MATCH_BANDS", 0)));
        k.bits_dw = num("SBM_BITS_DW", 0) == 2 ? 2 : (num("SBM_BITS_DW", 0) == 1 ? 1 : 0);
        return k;
    }();
    return t;
}

struct sbm_ctx {
    sbm_config cfg{};
    int n_simd = 1024; // SIMDs of the device (4 per CU): 1024 on a whole MI355X, fewer on a partitioned one
    int L = 0;
    hipStream_t stream = nullptr;
    int64_t cand_cap = 0;

    // templates
    int n_templates = 0;
    int64_t n_features = 0;
    std::vector<DevTL> h_tls;          // [n_templates][L]
    std::vector<uint32_t> h_fxy;
    std::vector<int32_t> h_class, h_tid;
    std::vector<int32_t> h_active;
    DevBuf d_tls, d_fxy, d_flabel, d_flevel, d_foff, d_class, d_tid, d_active, d_rawmin, d_rawkeep;
    DevBuf d_citems, d_cfoff, d_soff, d_soffbase; // coarse pass: per active template one record, its feature offsets sorted by byte
                                                   // misalignment, the first 64 of them again by slot (k_prep_coarse_items)
    bool citems_dirty = true;
    DevBuf d_fext;                      // per (template, level): largest feature x | largest feature y << 16 (k_mark_refine_tiles)
    DevBuf d_fxy_s, d_flabel_s, d_fcls; // refinement pass on the strip plane: features sorted by (x / T) & 15 per template level + 17 class offsets
    bool have_thr = false;
    float thr_cached = 0.f;
    // sbm_upload_templates_device (sbm_capi_install.inc): the ten tables above are built in this second set and change places
    // with the live ones once the kernels' verdict is in, so a refused call leaves the live set as it was; d_install is the
    // call's scratch (sbm_install_plan.h).  h_fxy is then not filled: features_in_bounds is its only reader, and it fetches
    // d_fxy on first need (ensure_host_fxy).
    struct TemplateTables {
        DevBuf tls, fxy, flabel, flevel, fxy_s, flabel_s, fcls, fext, cls, tid;
    } staged;
    DevBuf d_install;
    bool h_fxy_valid = true;

    // pyramid
    int rows[SBM_MAX_LEVELS]{}, cols[SBM_MAX_LEVELS]{};
    int channels = 0;
    int batch = 1;        // frames the per-level buffers, candidate lists and counters are allocated for
    int mask_frames = 1;  // masks d_mask[l], l >= 1, is allocated for: the batch's frames once a call brought a mask per frame
    // What the last match call (or build) left resident and what it launched: every later reader decides by it (sbm_call_record.h)
    static_assert(LF_MAX_LEVELS == SBM_MAX_LEVELS, "the record holds every level of the pyramid");
    CallRecord rec;
    int64_t lm_stride[SBM_MAX_LEVELS]{};
    DevBuf d_img[SBM_MAX_LEVELS], d_mask[SBM_MAX_LEVELS], d_quant[SBM_MAX_LEVELS], d_lm[SBM_MAX_LEVELS];
    // Levels that only the refinement pass reads (l < L-1) are built as ONE plane of spread bytes ("compact": an eighth
    // of the stores and of the HBM write-back; the refinement kernel applies the response LUT itself).  The 8-plane form
    // of such a level is materialised on demand for the stage entry points (ensure_full_lm).
    DevBuf d_lmc[SBM_MAX_LEVELS];
    // Coarsest level as BIT planes (round 4, sbm_coarse_bits.h): per frame 8 "response > 0" planes then 8 "response == 4"
    // planes, each lm_stride bits in the byte planes' flat order -- what the coarse pass reads (2 bits per position and
    // orientation instead of a byte)
    DevBuf d_blm;
    // Round 4: a T = 4 strip level that a match entry point builds is stored as BIT STRIPS instead (2 bits per cell and
    // orientation, build_lm_strip4_allty) and refined by k_similarity_local_bits (sbm_local_bits.h)
    DevBuf d_lbits[SBM_MAX_LEVELS];
    // ... and, as level 0 of a two-level pyramid, only in the tiles the call's coarse candidates read (LM_BIT_STRIPS_SPARSE):
    // one byte flag per frame and tile (sbm_refine_tiles.h), cleared with the counters, set by k_mark_refine_tiles
    DevBuf d_tiles;
    // ... and level 0's orientation map itself only where those tiles' strip builders read it (BuildPlan::sparse_gradient): the
    // source pass keeps the batch's level-0 source bytes here (batch x rows x cols x channels, packed), the gradient launch
    // behind the coarse pass reads them, and so does the whole launch that a later reader of d_quant[0] asks for
    // (ensure_level0_map) -- the caller's image may be gone by then (CallRecord::map0_whole, src0_ch).
    DevBuf d_src0;
    // ... and of that map only the work items the refinement can read (SBM_SPARSE_RECTS): per frame and band of RT_BAND pixel rows the
    // hull {xmin, xmax} of the map columns some candidate's refinement depends on, emptied where the tile flags are cleared, widened
    // by k_mark_refine_tiles, read by the sparse gradient launch.  Device data: a replayed graph follows each call's candidates.
    DevBuf d_rects;
    // ... and of those items the working ones, listed per frame by k_mark_refine_tiles for the launch to run from (SBM_SPARSE_LIST):
    // items_cap entries per frame, room for every item of the grid at any rows per item (CallRecord::sparse_list)
    DevBuf d_items;
    int64_t items_cap = 0;
    DevBuf d_sparse_items; // one int32: the working items of the last profiled sparse gradient launch (CallRecord::sparse_items)
    // ... and that copy is stored by the last match call enqueued on the context only (section 5 of DESIGN.md has the argument).
    // h_enqueued: a word of pinned host memory that one thread per launch reads in place (d_enqueued: its device address) --
    // match calls whose enqueue has ended (call_enqueued); d_call: CALL_WORDS words of device memory (sbm_lm_kernels.h) -- calls
    // executed, that count as last read, the source pass's note, the totals of sbm_get_source_retention.  call_counted: the launches of the call being enqueued
    // hold the one that counts it.  ev_call: recorded behind the last match call enqueued, on its stream (ensure_level0_map waits
    // for it); call_recorded: it was -- else that reader waits for the device.
    // sparse_src: the frames the call's sparse gradient launch reads -- the caller's own, or the retained copy.
    uint32_t* h_enqueued = nullptr;
    uint32_t* d_enqueued = nullptr;
    DevBuf d_call;
    bool call_counted = false;
    hipEvent_t ev_call = nullptr;
    bool call_recorded = false;
    FrameSource sparse_src;
    int refine_bits = -1; // sbm_set_refine_bits: -1 the process default (SBM_LOCAL_BITS, else on), 0 bytes, 1 bits
    DevBuf d_geo; // T[L], W[L], H[L] as int32 then stride[L] as int64
    bool foff_dirty = true;
    bool counters_fresh = false; // the linear-memory launch of this frame already reset the counters
    bool caller_work = false;    // a device entry point has enqueued on a caller's stream since the last device-wide wait

    // candidates / results
    DevBuf d_cands, d_counters, d_out, d_outcount;
    void* comm = nullptr;  // ncclComm_t of this context (sbm_comm_init)
    int comm_world = 0, comm_rank = 0;
    sbm_match_rec* mirror_out = nullptr; // optional device-visible mirror of the results (sbm_set_result_mirror)
    int32_t* mirror_count = nullptr;
    // host entry point (sbm_match): pinned result buffer the last kernel writes into (no device-to-host copy, one
    // synchronisation per call).  Caller frame buffers are pinned only on request (sbm_pin_host_buffer): the upload of
    // a frame inside such a range is one asynchronous DMA; any other host pointer takes the runtime's pageable path.
    sbm_match_rec* h_res = nullptr;
    int32_t* h_res_count = nullptr;
    int64_t h_res_cap = 0;
    struct PinnedRange {
        const uint8_t* p;
        size_t bytes;
    };
    std::vector<PinnedRange> pinned; // ranges THIS context registered and has not yet unregistered
    // host batch pipeline (sbm_match_batch_host_begin / _end): frames travel over PCIe on copy_stream into one of two
    // device input buffers while the kernels of the previous sub-batch run on `stream`; every sub-batch's match lists
    // land in one pinned host block through the result mirror
    hipStream_t copy_stream = nullptr;
    hipEvent_t ev_band[8] = {}; // sbm_match: the frame's upload in row bands, one event each
    DevBuf d_in[2], d_bout;
    DevBuf d_min[2]; // ... and the sub-batch's masks beside its frames (sbm_match_batch_host_begin_masked)
    hipEvent_t ev_up[2] = {}, ev_free[2] = {};
    uint8_t* h_bout = nullptr;
    size_t h_bout_bytes = 0;
    struct {
        bool active = false;
        int n_frames = 0;
        int64_t cap = 0;
    } pending;
    DevBuf d_scratch;
    // match epilogue + NMS (sbm_nms_batch_device): (class_idx, template_id) -> level-0 size table of the upload it was
    // built from (templates_gen), the scratch of frames whose lists exceed LDS, the host batch's kept lists
    uint64_t templates_gen = 0;
    uint64_t nms_labels_gen = ~(uint64_t)0;
    int nms_n_labels = 0;
    bool nms_labels_unique = true;
    DevBuf d_nms_labels, d_nms_scratch, d_nms_out;
    int32_t* h_nms_counts = nullptr;
    int h_nms_counts_frames = 0;
    // verify stage (sbm_capi_verify.inc): the patch set of the upload it was made for (verify_gen against templates_gen) -- the
    // sorted label table and the normalised bytes, on the device and on the host --, the {score, status} scratch of a call, grown
    // by the rule of d_nms_scratch, and the host sibling's frames, intermediate lists and pinned results
    uint64_t verify_gen = ~(uint64_t)0;
    std::vector<VerifyLabel> h_verify_labels;
    int64_t verify_patch_bytes = 0;
    DevBuf d_verify_labels, d_verify_patches, d_verify_scratch, d_verify_in, d_verify_lists;
    uint8_t* h_verify_out = nullptr;
    size_t h_verify_out_bytes = 0;
    // batched training (sbm_capi_train.inc): the scratch of a batch, grown by the rule of d_nms_scratch; the host form's images, masks and results
    DevBuf d_train, d_train_in, d_train_mask, d_train_out;
    // ragged training: the pinned slot the table of records (and a sweep's scale and coefficient tables) is copied from,
    // the event behind its last copy, and the sweep's scaled images, masks and tables
    void* h_train_table = nullptr;
    size_t h_train_table_cap = 0;
    hipEvent_t ev_train_table = nullptr;
    bool train_table_busy = false, train_table_recorded = false;
    hipStream_t train_table_stream = nullptr;
    DevBuf d_train_sweep;

    // hipGraph cache for sbm_match_device (one captured graph per distinct argument tuple)
    struct GraphEntry {
        GraphKey key; // sbm_frame_source.h
        hipGraph_t graph = nullptr;
        hipGraphExec_t exec = nullptr;
        uint64_t last_use = 0;
        CallRecord rec; // what the capture left in the context, taken once it has ended: a replay restores it (CallRecord::replayed)
    };
    std::vector<GraphEntry> graphs;
    uint64_t graph_clock = 0;
    int quantize_mode = 0, quantize_hs = 0; // sbm_set_quantize_mode
    int sparse_list_rows = -1;              // sbm_set_sparse_list_rows
    int pipeline_depth = 1;                 // sbm_set_pipeline_depth: batches the caller keeps in flight on this GPU
    int local_order = tuning().local_order; // -1 by the planes' size, 0 per-frame slots, 2 one frame-major list (sbm_set_refine_order)
    int coarse_mode = tuning().coarse;      // 0 auto (bit planes), 1 four waves per item, 2 one wave per item, 3 bit planes, 4 byte kernels by launch size (SBM_COARSE: A/B knob)
    // hipGraph replay of an entry point's launches (sbm_set_graph_mode): -1 auto (default) = the batch entry point and the
    // template-loop entry point replay a captured graph once the caller keeps several calls in flight
    // (sbm_set_pipeline_depth >= 2) and an argument tuple comes back; 0 never; 1 always (single frames too)
    int graph_pref = -1;
    bool auto_graph_off = false;      // auto: the caller's argument tuples never repeat (captures without hits): stop capturing
    int graph_captures_since_hit = 0;
    std::vector<GraphKey> graph_seen; // auto: tuples seen once (a tuple is captured at its second sighting)
    hipStream_t side = nullptr;
    hipEvent_t ev_fork[SBM_MAX_LEVELS] = {};
    hipEvent_t ev_join = nullptr;
    void drop_graphs()
    {
        for (auto& g : graphs) {
            (void)hipGraphExecDestroy(g.exec);
            (void)hipGraphDestroy(g.graph);
        }
        graphs.clear();
    }

    // profiling
    bool profiling = false;
    bool profiling_keep = false; // enabled == 2: timings accumulate over calls until they are read
    std::vector<Timing> timings;
    std::vector<float> timing_ms;

    hipEvent_t chain_event = nullptr;
    hipStream_t chain_stream = nullptr;
    void clear_timings()
    {
        for (auto& t : timings) {
            if (!t.shared_a) (void)hipEventDestroy(t.a);
            (void)hipEventDestroy(t.b);
        }
        timings.clear();
        timing_ms.clear();
        chain_event = nullptr;
        chain_stream = nullptr;
    }
};

namespace {

struct Scope { // optional per-kernel HIP-event bracket on the launch stream
    sbm_ctx* c;
    hipStream_t s;
    bool on;
    Timing t{};
    Scope(sbm_ctx* c_, hipStream_t s_, const char* name) : c(c_), s(s_), on(c_->profiling)
    {
        if (!on) return;
        t.name = name;
        // consecutive launches share one event: the end of the previous kernel is the start of this
        // one, so a single event packet sits between two kernels (as in an un-instrumented stream)
        if (c->chain_event && c->chain_stream == s) {
            t.a = c->chain_event;
            t.shared_a = true;
        } else {
            (void)hipEventCreate(&t.a);
            (void)hipEventRecord(t.a, s);
        }
        (void)hipEventCreate(&t.b);
    }
    ~Scope()
    {
        if (!on) return;
        (void)hipEventRecord(t.b, s);
        c->chain_event = t.b;
        c->chain_stream = s;
        c->timings.push_back(t);
    }
};

// Launch with exact kernel begin/end timestamps when profiling: hipExtLaunchKernelGGL stamps the
// dispatch packet itself (what rocprofv3's kernel trace reads), so no event packet sits between
// kernels and the measured durations are the kernels' own.
#define SBM_LAUNCH(ctx, name_, kernel, grid, block, smem, stream, ...)                                        \
    do {                                                                                                      \
        if ((ctx)->profiling) {                                                                               \
            Timing t_;                                                                                        \
            t_.name = name_;                                                                                  \
            (void)hipEventCreate(&t_.a);                                                                      \
            (void)hipEventCreate(&t_.b);                                                                      \
            hipExtLaunchKernelGGL(kernel, grid, block, smem, stream, t_.a, t_.b, 0, __VA_ARGS__);             \
            (ctx)->timings.push_back(t_);                                                                     \
        } else {                                                                                              \
            hipLaunchKernelGGL(kernel, grid, block, smem, stream, __VA_ARGS__);                               \
        }                                                                                                     \
    } while (0)

int check_level_dims(int rows, int cols, int T)
{
    if (rows <= 0 || cols <= 0 || T <= 0) return fail(SBM_ERR_INVALID, "bad level geometry %dx%d T=%d", rows, cols, T);
    if (rows % T || cols % T) // CV_Assert line2Dup.cpp:751-752
        return fail(SBM_ERR_INVALID, "level %dx%d is not a multiple of T=%d (linearize precondition)", rows, cols, T);
    if (((int64_t)rows * cols) % 16) // CV_Assert line2Dup.cpp:639
        return fail(SBM_ERR_INVALID, "level %dx%d: rows*cols %% 16 != 0 (computeResponseMaps precondition)", rows, cols);
    if ((int64_t)8 * lm_stride_for(rows, cols, T) >= (int64_t)INT32_MAX)
        return fail(SBM_ERR_INVALID, "level %dx%d too large for 32-bit linear-memory offsets", rows, cols);
    if (rows > 65535 || cols > 65535) return fail(SBM_ERR_INVALID, "image too large");
    return 0;
}

// bytes of one frame of level l stored as bit strips (lm_bits_offset) + a zero tail that covers a patch starting in it
int64_t lbits_frame_bytes(const sbm_ctx* c, int l)
{
    const int T = c->cfg.T[l], W = c->cols[l] / T, H = c->rows[l] / T;
    return (lm_bits_dwords(W, H) * 4 + (int64_t)H * 32 + 1024 + 255) / 256 * 256;
}

// (re)allocate the per-level buffers for a level-0 geometry
// frame_masks: the call brings one mask per frame, so levels >= 1 hold `frames` resized masks (else one)
int ensure_geometry(sbm_ctx* c, int rows, int cols, int channels, int frames = 1, bool frame_masks = false)
{
    if (channels != 1 && channels != 3) return fail(SBM_ERR_INVALID, "channels must be 1 or 3, got %d", channels);
    if (frames < 1 || frames > 65535) return fail(SBM_ERR_INVALID, "batch of %d frames out of range", frames);
    bool same = c->channels == channels && c->rows[0] == rows && c->cols[0] == cols && c->d_lm[c->L - 1].p && frames <= c->batch &&
                (frame_masks ? frames : 1) <= c->mask_frames;
    int r = rows, cc = cols;
    for (int l = 0; l < c->L; ++l) {
        if (l > 0) {
            r /= 2;
            cc /= 2;
        }
        if (int e = check_level_dims(r, cc, c->cfg.T[l])) return e;
        if (c->rows[l] != r || c->cols[l] != cc) same = false;
    }
    if (same) return 0;
    const size_t B = (size_t)std::max(frames, c->batch);
    const size_t MB = (size_t)std::max(frame_masks ? frames : 1, c->mask_frames);
    r = rows;
    cc = cols;
    for (int l = 0; l < c->L; ++l) {
        if (l > 0) {
            r /= 2;
            cc /= 2;
        }
        c->rows[l] = r;
        c->cols[l] = cc;
        c->lm_stride[l] = lm_stride_for(r, cc, c->cfg.T[l]);
        if (int e = c->d_img[l].ensure(B * r * cc * channels)) return e;
        if (int e = c->d_mask[l].ensure((l ? MB : 1) * r * cc)) return e; // level 0's: a host entry point's one uploaded mask
        if (int e = c->d_quant[l].ensure(B * r * cc)) return e;
        c->d_lm[l].release(); // fresh, zeroed: the tail past T*T*W*H must read as 0
        if (int e = c->d_lm[l].ensure(B * 8 * c->lm_stride[l], true)) return e;
        c->d_lmc[l].release();
        c->d_lbits[l].release(); // fresh, zeroed: the tail behind the bit strips must read as 0
        // (the coarsest level's plane: what the bit planes are packed from on grids the fused producer does not take)
        if (int e = c->d_lmc[l].ensure(B * c->lm_stride[l], true)) return e;
        if (l < c->L - 1) {
            if (c->cfg.T[l] == 4)
                if (int e = c->d_lbits[l].ensure(B * lbits_frame_bytes(c, l), true)) return e;
        }
        if (l == 0) {
            c->d_tiles.release(); // sized by level 0's grid and the batch
            if (c->d_lbits[0].p)
                if (int e = c->d_tiles.ensure(B * (size_t)refine_tile_count(cc / c->cfg.T[0], r / c->cfg.T[0]), true)) return e;
            c->d_src0.release();
            if (c->d_tiles.p && c->L == 2 && tuning().sparse_gradient)
                if (int e = c->d_src0.ensure(B * r * cc * channels)) return e;
            c->d_rects.release();
            if (c->d_src0.p && tuning().sparse_rects)
                if (int e = c->d_rects.ensure(B * (size_t)refine_band_count(r) * 2 * sizeof(int32_t), true)) return e; // zeroed: every band empty
            c->d_items.release();
            c->items_cap = 0;
            if (c->d_rects.p && tuning().sparse_list) {
                const int64_t cap = refine_list_capacity(r, cc, QS_USEFUL);
                if (cap < (int64_t)1 << 24) { // (else: no lists, every wave tests its own item)
                    if (int e = c->d_items.ensure(B * (size_t)refine_list_stride(cap) * sizeof(int32_t))) return e;
                    // no list anywhere until a reset says so too
                    HIP_TRY(hipMemset(c->d_items.p, 0xff, B * (size_t)refine_list_stride(cap) * sizeof(int32_t)));
                    HIP_TRY(hipStreamSynchronize(nullptr)); // (as in DevBuf::ensure: before anything is enqueued behind it)
                    c->items_cap = cap;
                }
            }
            if (c->d_src0.p)
                if (int e = c->d_sparse_items.ensure(256, true)) return e;
        }
        c->rec.forms[l].forget();
    }
    c->d_blm.release(); // fresh, zeroed: the tails of the bit planes must read as 0 too
    if (int e = c->d_blm.ensure(B * 2 * c->lm_stride[c->L - 1] + 256, true)) return e;
    if (B > (size_t)c->batch) { // per-frame candidate lists and counters
        if (int e = c->d_cands.ensure(B * c->cand_cap * sizeof(Cand))) return e;
        c->d_counters.release();
        if (int e = c->d_counters.ensure(B * CTR_STRIDE * sizeof(int32_t) + 256, true)) return e;
        c->batch = (int)B;
    }
    c->mask_frames = (int)MB;
    c->channels = channels;
    c->foff_dirty = true;
    c->rec.levels_valid = 0;
    c->rec.map0_whole = true; // nothing resident: nothing to complete
    c->drop_graphs(); // captured launches hold the old buffer addresses
    return 0;
}

int ensure_level(sbm_ctx* c, int l, int rows, int cols)
{
    if (int e = check_level_dims(rows, cols, c->cfg.T[l])) return e;
    if (c->rows[l] == rows && c->cols[l] == cols && c->d_lm[l].p && c->d_quant[l].p) return 0;
    c->drop_graphs();
    c->rows[l] = rows;
    c->cols[l] = cols;
    c->lm_stride[l] = lm_stride_for(rows, cols, c->cfg.T[l]);
    if (int e = c->d_quant[l].ensure((size_t)rows * cols)) return e;
    c->d_lm[l].release();
    if (int e = c->d_lm[l].ensure((size_t)8 * c->lm_stride[l], true)) return e;
    c->d_lmc[l].release();
    c->d_lbits[l].release();
    if (l == 0) {
        c->d_tiles.release();
        c->d_src0.release();
        c->d_rects.release();
        c->d_items.release();
        c->items_cap = 0;
        c->rec.map0_whole = true; // the caller sets the whole map
    }
    c->rec.forms[l].forget();
    if (l == c->L - 1) {
        c->d_blm.release();
        if (int e = c->d_blm.ensure((size_t)2 * c->lm_stride[l] + 256, true)) return e;
    }
    c->foff_dirty = true;
    // This level now holds ONE frame of a geometry the other per-level buffers (next level's image, mask, compact
    // plane, the batch's frames) were not sized for: the next ensure_geometry() must not take its `same` fast path.
    c->channels = 0;
    return 0;
}

int upload_geo(sbm_ctx* c, hipStream_t s)
{
    const int L = c->L;
    std::vector<int32_t> g(3 * SBM_MAX_LEVELS);
    std::vector<int64_t> st(SBM_MAX_LEVELS);
    for (int l = 0; l < L; ++l) {
        g[l] = c->cfg.T[l];
        g[SBM_MAX_LEVELS + l] = c->cols[l] / c->cfg.T[l];
        g[2 * SBM_MAX_LEVELS + l] = c->rows[l] / c->cfg.T[l];
        st[l] = c->lm_stride[l];
    }
    const size_t gi = g.size() * sizeof(int32_t), gs = st.size() * sizeof(int64_t);
    if (int e = c->d_geo.ensure(gi + gs)) return e;
    HIP_TRY(hipMemcpyAsync(c->d_geo.p, g.data(), gi, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync((char*)c->d_geo.p + gi, st.data(), gs, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s)); // host vectors go out of scope
    return 0;
}

// Which gradient kernel a launch gets.  The row-streaming kernel (sbm_quantize_stream.h) is the throughput form: a wave
// walks a 256-column strip for tens of rows, so a launch needs thousands of waves to fill the chip and a single small
// frame would be a few long serial chains; the tile kernel (k_quantize) is the latency form (1024 short-lived tiles
// per Mpixel) and the only one with the float outputs and arbitrary widths.  SBM_QUANTIZE=tile|stream forces one for
// A/B runs, SBM_QS_HS sets the rows per wave.
// segment lanes of the packed last strip (0: none); SBM_QS_PACK=0 is the A/B knob
static int qs_pack_lanes(int rows, int cols, const FrameSource& src, const MaskSource& mask)
{
    if (!source_may_pack(src)) return 0;
    const int lanes = tuning().qs_pack ? quantize_stream_pack_lanes(rows, cols, src.ch, src.frames, kernel_mask_stride(mask)) : 0;
    if (!lanes) return 0;
    // the frames of a group are addressed by 32-bit per-lane offsets from the group's first frame: the caller's frame
    // stride (any value, also negative or zero) must keep them within 2 GiB
    const int64_t span = (int64_t)(64 / lanes - 1) * src.frame_stride;
    if (src.frame_stride < 0 || span + (int64_t)rows * src.stride >= (int64_t)0x7ff00000) return 0;
    return lanes;
}

// rows = the image's rows; band_rows = the output rows of this launch (rows for a whole level; a row band of a
// build-sharded step otherwise, which always takes the streaming kernel: the tile kernel has no row-range form)
// wf: the launch has float outputs
int quantize_stream_rows(const sbm_ctx* c, int rows, int cols, const FrameSource& src, const MaskSource& mask, bool wf, int band_rows = 0)
{
    const int ch = src.ch, frames = src.frames;
    const bool band = band_rows > 0 && band_rows < rows;
    const int out_rows = band ? band_rows : rows;
    const int mode = c->quantize_mode ? c->quantize_mode : tuning().quantize;
    const int env_hs = (int64_t)rows * cols >= (1 << 20) ? tuning().hs0 : tuning().hs1;
    const int force_hs = c->quantize_hs ? c->quantize_hs : env_hs;
    if (wf || (mode == 1 && !band) || cols < 4 || (cols & 3) || (int64_t)rows * cols >= (int64_t)0x7ff00000) return 0;
    const int64_t strips = (cols + QS_USEFUL - 1) / QS_USEFUL;
    if (force_hs > 0) return (force_hs + 1) & ~1;
    // One batch at a time, a SIMD needs its full set of resident waves (3 at the BGR kernel's register count, 6 for gray) to
    // hide the scalar bookkeeping and dependency bubbles of each: a launch alone on the chip takes about
    // ceil(waves / resident slots) x (hs + 10 halo rows), and the latency branch below minimises that.
    const int64_t slots = (int64_t)c->n_simd * (ch == 3 ? 3 : 6); // resident waves: 3 per SIMD at the BGR kernel's registers, 6 gray
    // waves per row block: one per strip and frame, except that a narrow last strip is shared by several frames
    const int pack = qs_pack_lanes(rows, cols, src, mask);
    const int64_t per_rb = pack ? (strips - 1) * frames + (frames + 64 / pack - 1) / (64 / pack) : strips * frames;
    // a work item runs whole groups of 7 row iterations (sbm_quantize_stream.h): rows + 10 warm-up / drain, rounded up
    // (sbm_quantize_rows_plan.h has the arithmetic of both branches)
    int hs;
    if (c->pipeline_depth >= 2) {
        // Throughput sizing (the caller keeps several batches in flight on other streams / contexts, sbm_set_pipeline_depth).
        // The 10 warm-up / drain rows of every work item are pure overhead, so the launch's TOTAL work, waves x row iterations,
        // asks for few long items, at most 42 iterations (profiles/r03_rows_per_item_sweep.txt) -- but only down to one wave
        // per SIMD.  The step is no longer bound by vector issue (the whole step issues about 0.6 of the ceiling), the launches
        // of a call are a chain, and the other batches' kernels do NOT take up what a launch of fewer waves than SIMDs leaves
        // idle: level 1 of 16 x 1024^2 x 3 at 32 rows is 576 waves of 42 iterations and lasts 62.1 us pipelined, at 18 rows 1044
        // waves of 28 iterations and 50.5 us, and that alone takes 2.0 us off a step of 73.2; 12 rows lose and 10 rows tie with
        // 32 (profiles/gradient_item_sizing.txt, sections 1, 4, 5).  So: the least total work among the launches that have a
        // wave for every SIMD.  A launch that has them at its least-work size keeps that size (level 0 of that batch: 2240 waves at 32 rows).
        hs = qs_rows_throughput(per_rb, out_rows, c->n_simd);
    } else {
        // Latency sizing: every work item resident at once, as few row iterations as that allows
        hs = qs_rows_latency(per_rb, out_rows, slots);
    }
    // small launches: the 16 x 64 tiles of k_quantize finish sooner than a few long serial chains
    if (!band && mode != 2 && (int64_t)rows * cols * frames < ((int64_t)4 << 20)) return 0;
    return hs;
}

// A reduced form of the streaming kernel's row loop (QSStage): the source pass with its retained copy, or the gradient of
// the flagged tiles' reach.  Whole levels only, no mask; the caller has checked that the launch takes the streaming kernel.
struct QSForm {
    int stage;
    uint8_t* keep;
    int64_t keep_fs;
    const uint8_t* tile_flags;
    int n_tiles, T, W, H;
    const int32_t* need_rects = nullptr; // QS_SPARSE: the record of need rectangles, n_bands pairs per frame; null: the tile-driven items
    int n_bands = 0;
    int32_t* item_count = nullptr;       // QS_SPARSE: where the working items are counted (profiling), or null
    // QS_SPARSE by slots (sparse_list_plan): the frames' lists of working items and the grid they were made for; slots 0: a wave per item
    const int32_t* item_list = nullptr;
    int64_t list_stride = 0;
    // (fixed_hs, list_n_full: the launch's own grid as the plan saw it; list_hs: the rows per item of the grid the lists' entries name)
    int list_cap = 0, slots = 0, fixed_hs = 0, list_n_full = 0, list_hs = 0;
    // QS_SOURCE: the call counters the work items decide by whether they store the copy, and where the decision is noted (QSArgs)
    const uint32_t* call_enqueued = nullptr;
    const uint32_t* call_executed = nullptr;
    uint32_t* call_note = nullptr;
};

// rows per work item of the source pass: its items run hs + 3 row iterations, in whole groups of 6
int source_pass_rows() { return tuning().src_hs > 0 ? (tuning().src_hs + 1) & ~1 : 32; }

// One launch of the gradient stage: where its frames and masks lie, the level's geometry, the outputs, the rows
struct QuantizeLaunch {
    FrameSource src;
    MaskSource mask;            // none: every pixel counts
    int rows = 0, cols = 0;
    float weak = 0.f;
    uint8_t* out = nullptr;     // the orientation map, rows x cols per frame (packed)
    float* mag = nullptr;       // float outputs (the stage entry points, training): the tile kernel
    float* ori = nullptr;
    uint8_t* pyr = nullptr;     // the fused cv::pyrDown output, (rows / 2) x (cols / 2) x ch per frame (packed), or null
    int row_lo = 0, row_hi = -1; // output rows [row_lo, row_hi); -1: to the last
    bool tile_band = false;
    const QSForm* form = nullptr;
};

int launch_quantize(sbm_ctx* c, hipStream_t s, const QuantizeLaunch& q)
{
    const FrameSource& src = q.src;
    const int rows = q.rows, cols = q.cols, ch = src.ch, frames = src.frames, row_lo = q.row_lo, row_hi = q.row_hi < 0 ? rows : q.row_hi;
    const QSForm* const form = q.form;
    const bool tile_band = q.tile_band;
    const bool band = row_lo > 0 || row_hi < rows;
    // The table forms (sbm_match_batch_device_ptrs: a device array of frame addresses; sbm_match_batch_device_planes: of three plane
    // addresses per frame, three channels, `stride` a plane's row), with the masks, if any, in a device array of mask addresses.
    // The caller's level-0 launch only -- whole, without float outputs.
    const bool planes = src.kind == FRAMES_PLANES;
    const bool table = frames_in_table(src);
    if (table && (band || tile_band || q.mag || q.ori || (q.mask.kind != MASK_NONE && q.mask.kind != MASK_TABLE) || (form && form->stage != QS_SOURCE)))
        return fail(SBM_ERR_STATE, "a table of frame pointers names the frames of a whole level-0 launch only");
    if (planes && ch != FPL_CHANNELS) return fail(SBM_ERR_STATE, "a table of plane pointers names frames of three channels");
    if (!table && q.mask.kind == MASK_TABLE) return fail(SBM_ERR_STATE, "a table of mask pointers needs a table of frame pointers");
    // what the kernels get: the frames or their table, the strides a table form does not read as 0
    const uint8_t* const d_img = (const uint8_t*)src.base;
    const uint8_t* const d_mask = (const uint8_t*)q.mask.base;
    const int stride = src.stride;
    const int64_t img_fs = kernel_frame_stride(src), mask_fs = kernel_mask_stride(q.mask);
    uint8_t* const d_out = q.out;
    float* const d_mag = q.mag;
    float* const d_ori = q.ori;
    uint8_t* const d_pyr = q.pyr;
    // tile_band: rows [row_lo, row_hi) as a band of whole rows of 16 x 64 TILES (row_lo a multiple of 16, row_hi too or the
    // last row): the latency path of sbm_match, whose level-0 launches follow the frame's upload band by band
    const int tile_row0 = tile_band ? row_lo / QT_R : 0;
    dim3 grid((cols + QT_C - 1) / QT_C, tile_band ? (row_hi - row_lo + QT_R - 1) / QT_R : (rows + QT_R - 1) / QT_R, frames);
    const float thr_sq = q.weak * q.weak;
    const bool wf = d_mag || d_ori;
    const int64_t out_fs = (int64_t)rows * cols, pyr_fs = (int64_t)(rows / 2) * (cols / 2) * ch; // the context's own per-frame buffers
    int hs = tile_band ? 0 : quantize_stream_rows(c, rows, cols, src, q.mask, wf, band ? row_hi - row_lo : 0);
    if (form && (!hs || band || d_mask)) return fail(SBM_ERR_STATE, "a reduced gradient form needs a whole, unmasked launch of the streaming kernel");
    if (form && form->stage == QS_SOURCE) hs = source_pass_rows();
    // The source pass as whole lines (sbm_source_lines.h) wherever the caller's layout admits it; every other layout -- a row pad
    // of 13 bytes, an odd frame stride -- stays with the strided form below.
    if (form && form->stage == QS_SOURCE && source_takes_lines(src, rows, cols, tuning().source_lines)) {
        QSArgs a;
        memset(&a, 0, sizeof a);
        a.img = d_img;
        a.pyr = d_pyr;
        a.img_fs = img_fs;
        a.pyr_fs = pyr_fs;
        a.rows = rows;
        a.cols = cols;
        a.stride = stride;
        a.hs = hs;
        a.row_lo = 0;
        a.row_hi = rows;
        a.n_strips = sl_strips(cols);
        a.n_rblocks = sl_row_blocks(0, rows, hs);
        a.frames = frames;
        a.keep = form->keep;
        a.keep_fs = form->keep_fs;
        a.call_enqueued = form->call_enqueued, a.call_executed = form->call_executed, a.call_note = form->call_note;
        const dim3 g((unsigned)((sl_items(cols, a.n_rblocks, frames) + 3) / 4));
        if (table && ch == 1) SBM_LAUNCH(c, "k_quantize", (k_source_lines_ptrs<1>), g, dim3(256), 0, s, a);
        else if (table) SBM_LAUNCH(c, "k_quantize", (k_source_lines_ptrs<3>), g, dim3(256), 0, s, a);
        else if (ch == 1) SBM_LAUNCH(c, "k_quantize", (k_source_lines<1>), g, dim3(256), 0, s, a);
        else SBM_LAUNCH(c, "k_quantize", (k_source_lines<3>), g, dim3(256), 0, s, a);
        HIP_TRY(hipGetLastError());
        c->rec.source_form = 2;
        return 0;
    }
    if (hs) {
        QSArgs a;
        memset(&a, 0, sizeof a);
        a.img = d_img;
        a.mask = d_mask;
        a.out = d_out;
        a.pyr = d_pyr;
        a.img_fs = img_fs;
        a.out_fs = out_fs;
        a.pyr_fs = pyr_fs;
        a.mask_fs = mask_fs;
        a.rows = rows;
        a.cols = cols;
        a.stride = stride;
        a.thr_i = thr_sq < 2147483000.f ? (int)floorf(thr_sq) : INT_MAX; // mag is an integer: mag > weak^2 <=> mag > floor(weak^2)
        a.hs = hs;
        a.row_lo = row_lo;
        a.row_hi = row_hi;
        a.n_strips = (cols + QS_USEFUL - 1) / QS_USEFUL;
        a.n_rblocks = (row_hi - row_lo + hs - 1) / hs;
        a.frames = frames;
        a.pack_lanes = qs_pack_lanes(rows, cols, src, q.mask);
        a.pack_groups = a.pack_lanes ? (frames + 64 / a.pack_lanes - 1) / (64 / a.pack_lanes) : 0;
        const int stage = form ? form->stage : (int)QS_WHOLE;
        if (stage == QS_SOURCE) {
            a.keep = form->keep;
            a.keep_fs = form->keep_fs;
            a.call_enqueued = form->call_enqueued, a.call_executed = form->call_executed, a.call_note = form->call_note;
        } else if (stage == QS_SPARSE) {
            a.pyr = nullptr;
            a.tile_flags = form->tile_flags;
            a.n_tiles = form->n_tiles;
            a.grid_t = form->T;
            a.grid_w = form->W;
            a.grid_h = form->H;
            a.item_count = form->item_count;
            if (form->need_rects) {
                // an item is (k-th strip from the left end of its rows' hull, row block, frame); the packed last strip stays fixed
                a.need_rects = form->need_rects;
                a.n_bands = form->n_bands;
            }
            if (form->slots > 0) {
                // (the lists were made for one grid: the one this launch runs)
                if (form->fixed_hs != hs || form->list_n_full != (a.pack_lanes ? a.n_strips - 1 : a.n_strips) || !form->need_rects ||
                    form->list_hs < 2 || (form->list_hs & 1))
                    return fail(SBM_ERR_STATE, "the lists of working items were made for another grid than the sparse gradient launch runs");
                a.item_list = form->item_list;
                a.list_stride = form->list_stride;
                a.list_cap = form->list_cap;
                a.slots = form->slots;
                a.list_hs = form->list_hs;
                a.list_n_rblocks = (rows + form->list_hs - 1) / form->list_hs;
            }
            c->rec.sparse_items[0] = form->need_rects ? 2 : 1;
            c->rec.sparse_items[1] = -1;
            c->rec.sparse_items[2] = a.slots > 0 ? frames * a.slots + quantize_slots_packed(a) : quantize_stream_items(a);
            c->rec.sparse_items_pending = form->item_count != nullptr;
            c->rec.sparse_list[0] = a.slots > 0, c->rec.sparse_list[1] = a.slots, c->rec.sparse_list[2] = a.slots > 0 ? a.list_hs : 0;
        }
        const dim3 g((unsigned)(a.slots > 0 ? quantize_slots_groups(a) : (quantize_stream_items(a) + 3) / 4));
        // (one timing name for all three forms: the launches of the gradient stage)
#define SBM_QS(CH_)                                                                                                         \
        do {                                                                                                                \
            if (stage == QS_SOURCE) SBM_LAUNCH(c, "k_quantize", (k_quantize_stream<CH_, QS_SOURCE>), g, dim3(256), 0, s, a); \
            else if (stage == QS_SPARSE && a.slots > 0) SBM_LAUNCH(c, "k_quantize", (k_quantize_stream_slots<CH_>), g, dim3(256), 0, s, a); \
            else if (stage == QS_SPARSE) SBM_LAUNCH(c, "k_quantize", (k_quantize_stream<CH_, QS_SPARSE>), g, dim3(256), 0, s, a); \
            else SBM_LAUNCH(c, "k_quantize", (k_quantize_stream<CH_, QS_WHOLE>), g, dim3(256), 0, s, a);                     \
        } while (0)
        // (the table forms have the whole row loop and the source pass; the sparse launch reads the retained copy)
#define SBM_QS_PTRS(CH_)                                                                                                    \
        do {                                                                                                                \
            if (stage == QS_SOURCE) SBM_LAUNCH(c, "k_quantize", (k_quantize_stream_ptrs<CH_, QS_SOURCE>), g, dim3(256), 0, s, a); \
            else SBM_LAUNCH(c, "k_quantize", (k_quantize_stream_ptrs<CH_, QS_WHOLE>), g, dim3(256), 0, s, a);                \
        } while (0)
        switch (src.kind) {
        case FRAMES_PLANES:
            if (stage == QS_SOURCE) SBM_LAUNCH(c, "k_quantize", (k_quantize_stream_planes<QS_SOURCE>), g, dim3(256), 0, s, a);
            else SBM_LAUNCH(c, "k_quantize", (k_quantize_stream_planes<QS_WHOLE>), g, dim3(256), 0, s, a);
            break;
        case FRAMES_TABLE:
            if (ch == 1) SBM_QS_PTRS(1);
            else SBM_QS_PTRS(3);
            break;
        case FRAMES_STRIDED:
            if (ch == 1) SBM_QS(1);
            else SBM_QS(3);
            break;
        }
#undef SBM_QS_PTRS
#undef SBM_QS
        HIP_TRY(hipGetLastError());
        if (stage == QS_SOURCE) c->rec.source_form = 1;
        return 0;
    }
    if (band && !tile_band) return fail(SBM_ERR_INVALID, "a row band needs the streaming gradient kernel (cols %% 4 == 0, no float outputs)");
    if (tile_band && (row_lo % QT_R || (row_hi % QT_R && row_hi != rows))) return fail(SBM_ERR_INVALID, "a band of tiles must start and end on tile rows");
    // many tiles per CU (a batch of frames): 512-thread blocks, four of them per CU; else 1024-thread blocks (tile latency)
    const bool many = (int64_t)grid.x * grid.y * grid.z >= 2048;
    // (the table forms: d_img / d_mask are the tables)
#define SBM_QUANTIZE(CH_, WF_, PTRS_, PLANES_)                                                                              \
    do {                                                                                                                    \
        if (many)                                                                                                           \
            SBM_LAUNCH(c, "k_quantize", (k_quantize<CH_, WF_, QN_THROUGHPUT, PTRS_, PLANES_>), grid, dim3(QN_THROUGHPUT), 0, s, d_img, rows, cols, \
                       stride, d_mask, thr_sq, d_out, d_mag, d_ori, d_pyr, img_fs, out_fs, pyr_fs, tile_row0, mask_fs);     \
        else                                                                                                                \
            SBM_LAUNCH(c, "k_quantize", (k_quantize<CH_, WF_, QN_LATENCY, PTRS_, PLANES_>), grid, dim3(QN_LATENCY), 0, s, d_img, rows, cols, stride, \
                       d_mask, thr_sq, d_out, d_mag, d_ori, d_pyr, img_fs, out_fs, pyr_fs, tile_row0, mask_fs);             \
    } while (0)
    switch (src.kind) {
    case FRAMES_PLANES: SBM_QUANTIZE(3, false, true, true); break;
    case FRAMES_TABLE:
        if (ch == 1) SBM_QUANTIZE(1, false, true, false);
        else SBM_QUANTIZE(3, false, true, false);
        break;
    case FRAMES_STRIDED:
        if (ch == 1 && !wf) SBM_QUANTIZE(1, false, false, false);
        else if (ch == 1) SBM_QUANTIZE(1, true, false, false);
        else if (!wf) SBM_QUANTIZE(3, false, false, false);
        else SBM_QUANTIZE(3, true, false, false);
        break;
    }
#undef SBM_QUANTIZE
    HIP_TRY(hipGetLastError());
    return 0;
}

// the register-only linear-memory kernel handles the reference's strides on 16-byte aligned rows
bool lm_rows_ok(const uint8_t* d_q, int cols, int T)
{
    return (T == 4 || T == 8) && ((cols / T) & 3) == 0 && (cols & 15) == 0 && (((uintptr_t)d_q) & 15) == 0;
}

// every level takes the one-launch builder k_build_lm_rows
bool all_rows_ok(const sbm_ctx* c)
{
    for (int l = 0; l < c->L; ++l)
        if (!lm_rows_ok(c->d_quant[l].as<uint8_t>(), c->cols[l], c->cfg.T[l])) return false;
    return true;
}

// A batch of frames on this pyramid takes the batched any-stride builder k_build_lm_any (sbm_lm_any.h): some level is off
// the one-launch builder's grid, and every stride is one that kernel's LDS tiles are sized for
bool any_batch_ok(const sbm_ctx* c)
{
    if (all_rows_ok(c)) return false;
    for (int l = 0; l < c->L; ++l)
        if (c->cfg.T[l] > LMA_MAX_T) return false;
    return true;
}

// what the form of every level's linear memories follows from (sbm_level_forms.h)
PlanInputs plan_inputs(const sbm_ctx* c)
{
    PlanInputs p;
    p.L = c->L;
    for (int l = 0; l < c->L; ++l) {
        p.T[l] = c->cfg.T[l];
        p.rows[l] = c->rows[l];
        p.cols[l] = c->cols[l];
        p.has_spread[l] = c->d_lmc[l].p != nullptr;
        p.has_bit_strips[l] = c->d_lbits[l].p != nullptr;
    }
    p.has_bit_planes = c->d_blm.p != nullptr;
    p.coarse_mode = c->coarse_mode;
    p.refine_bits = c->refine_bits;
    p.have_thr = c->have_thr;
    p.thr = c->thr_cached;
    p.full_lm = tuning().full_lm;
    p.strip_lm = tuning().strip_lm;
    p.lm_allty = tuning().lm_allty;
    p.fused_bits = tuning().fused_bits;
    p.local_bits = tuning().local_bits;
    p.sparse_strips = tuning().sparse_strips && c->d_tiles.p != nullptr;
    return p;
}
bool coarse_on_bits(const sbm_ctx* c) { return coarse_on_bits(plan_inputs(c)); }

// One level's share of a k_build_lm_rows launch that makes it in form f, from block `begin` on; *blocks: its 256-thread blocks
LmLevelArgs lm_level_args(const sbm_ctx* c, int l, LmForm f, int frames, int begin, int* blocks)
{
    const int T = c->cfg.T[l], W = c->cols[l] / T, H = c->rows[l] / T;
    const int64_t stride = c->lm_stride[l];
    // few frames: shorter, more numerous work items
    const LmWork w = lm_work(f, T, c->rows[l], W, H, frames < 4 ? LM_FULL_SPLIT : 1, tuning().lm_allty);
    const bool strips = f == LM_BIT_STRIPS || f == LM_BIT_STRIPS_SPARSE; // one layout: the kernel's compact == 4
    uint8_t* const lm = f == LM_PLANES8 ? c->d_lm[l].as<uint8_t>() : f == LM_BIT_PLANES ? c->d_blm.as<uint8_t>()
                      : strips ? c->d_lbits[l].as<uint8_t>() : c->d_lmc[l].as<uint8_t>();
    const int64_t lm_fs = strips ? lbits_frame_bytes(c, l) : (f == LM_PLANES8 ? 8 : f == LM_BIT_PLANES ? 2 : 1) * stride;
    *blocks = (int)((w.items + 255) / 256);
    return LmLevelArgs{c->d_quant[l].as<uint8_t>(), lm, stride, c->rows[l], c->cols[l], W, H, T, begin, (int64_t)c->rows[l] * c->cols[l], lm_fs,
                       strips ? (int32_t)LM_BIT_STRIPS : (int32_t)f, w.split, w.allty};
}

// level l alone (frame 0) in form f through the one-launch builder
int launch_lm_level(sbm_ctx* c, hipStream_t s, int l, LmForm f)
{
    LmArgs a;
    memset(&a, 0, sizeof a);
    a.n_levels = 1;
    int blocks = 0;
    a.lv[0] = lm_level_args(c, l, f, 1, 0, &blocks);
    SBM_LAUNCH(c, "k_build_lm", k_build_lm_rows, dim3((unsigned)blocks), dim3(256), 0, s, a);
    HIP_TRY(hipGetLastError());
    c->rec.note_level_build(l, f, 1, a.lv[0].split, a.lv[0].allty);
    return 0;
}

// the 8 response planes of level l (frame 0) from its resident orientation map
int launch_build_lm(sbm_ctx* c, hipStream_t s, int l)
{
    const uint8_t* d_q = c->d_quant[l].as<uint8_t>();
    uint8_t* d_lm = c->d_lm[l].as<uint8_t>();
    const int rows = c->rows[l], cols = c->cols[l], T = c->cfg.T[l], W = cols / T, H = rows / T;
    const int64_t lm_stride = c->lm_stride[l];
    if (lm_rows_ok(d_q, cols, T)) return launch_lm_level(c, s, l, LM_PLANES8);
    if (T <= 8) {
        const int tw = LM_GX * T, lw = tw + T - 1, lwp = (lw + 3) & ~3, lh = 2 * T - 1;
        const size_t smem = (size_t)lh * lwp + (size_t)lh * tw + (size_t)T * T * LM_GX;
        dim3 grid((W + LM_GX - 1) / LM_GX, H);
        SBM_LAUNCH(c, "k_build_lm", k_build_lm, grid, dim3(256), smem, s, d_q, rows, cols, T, W, H, d_lm, lm_stride);
        HIP_TRY(hipGetLastError());
        c->rec.note_level_build(l, LM_PLANES8, 3);
        return 0;
    }
    // large strides: unfused path through scratch (spread, 8 response maps)
    const int64_t n = (int64_t)rows * cols;
    if (int e = c->d_scratch.ensure((size_t)9 * n)) return e;
    uint8_t* sp = c->d_scratch.as<uint8_t>();
    uint8_t* maps = sp + n;
    const int blocks = (int)std::min<int64_t>((n + 255) / 256, 4096);
    Scope sc(c, s, "k_build_lm_unfused");
    hipLaunchKernelGGL(k_spread, dim3(blocks), dim3(256), 0, s, d_q, rows, cols, T, sp);
    hipLaunchKernelGGL(k_response, dim3(blocks), dim3(256), 0, s, sp, n, maps);
    for (int o = 0; o < 8; ++o)
        hipLaunchKernelGGL(k_linearize, dim3(blocks), dim3(256), 0, s, maps + o * n, rows, cols, T, d_lm + o * lm_stride);
    HIP_TRY(hipGetLastError());
    c->rec.note_level_build(l, LM_PLANES8, 4);
    return 0;
}

// 8-plane linear memories of level l (frame 0) for the stage entry points: expanded from the spread plane, or -- a level held
// as bit strips or bit planes only -- from the orientation map, which is still resident
int ensure_level0_map(sbm_ctx* c, hipStream_t s);
int ensure_full_lm(sbm_ctx* c, int l, hipStream_t s)
{
    const LmForm src = full_lm_source(c->rec.forms[l]);
    // nothing current: the level's strips were built sparsely (or nothing was built yet: not resident, nothing to do)
    if (src == LM_PLANES8 || (src == LM_NONE && l >= c->rec.levels_valid)) return 0;
    if (l == 0 && src != LM_SPREAD && src != LM_SPREAD_STRIP) // built from the map, which a sparse call left in pieces
        if (int e = ensure_level0_map(c, s)) return e;
    if (src == LM_SPREAD || src == LM_SPREAD_STRIP) {
        const int T = c->cfg.T[l];
        const int64_t n = (int64_t)T * T * (c->cols[l] / T) * (c->rows[l] / T);
        hipLaunchKernelGGL(k_expand_lm, dim3((unsigned)std::min<int64_t>((n / 4 + 255) / 256, 4096)), dim3(256), 0, s, c->d_lmc[l].as<uint8_t>(), n,
                           c->d_lm[l].as<uint8_t>(), c->lm_stride[l], src == LM_SPREAD_STRIP ? 1 : 0, c->cols[l] / T, c->rows[l] / T);
        HIP_TRY(hipGetLastError());
    } else if (int e = launch_build_lm(c, s, l)) return e;
    c->rec.forms[l].planes8 = true;
    return 0;
}

// (raw_thresholds: sbm_frame_plan.h -- the tables of a frame plan are made with the same function)
int ensure_thresholds(sbm_ctx* c, float thr, hipStream_t s)
{
    if (c->have_thr && memcmp(&thr, &c->thr_cached, sizeof thr) == 0) return 0;
    const size_t n = (size_t)c->n_templates * c->L;
    std::vector<int32_t> gt(n), ge(n);
    for (size_t i = 0; i < n; ++i) raw_thresholds(c->h_tls[i].nf, thr, &gt[i], &ge[i]);
    if (int e = c->d_rawmin.ensure(n * 4)) return e;
    if (int e = c->d_rawkeep.ensure(n * 4)) return e;
    HIP_TRY(hipMemcpyAsync(c->d_rawmin.p, gt.data(), n * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(c->d_rawkeep.p, ge.data(), n * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    c->thr_cached = thr;
    c->have_thr = true;
    c->citems_dirty = true;
    return 0;
}

int ensure_foff(sbm_ctx* c, hipStream_t s)
{
    if (!c->foff_dirty || c->n_features == 0) return 0;
    if (int e = upload_geo(c, s)) return e;
    const int32_t* g = c->d_geo.as<int32_t>();
    const int64_t* st = (const int64_t*)((char*)c->d_geo.p + 3 * SBM_MAX_LEVELS * sizeof(int32_t));
    const int blocks = (int)std::min<int64_t>((c->n_features + 255) / 256, 8192);
    SBM_LAUNCH(c, "k_prep_features", k_prep_features, dim3(blocks), dim3(256), 0, s, c->d_fxy.as<uint32_t>(),
                       c->d_flabel.as<uint8_t>(), c->d_flevel.as<uint8_t>(), c->n_features, g,
                       g + SBM_MAX_LEVELS, g + 2 * SBM_MAX_LEVELS, st, c->d_foff.as<int32_t>(), c->L - 1);
    HIP_TRY(hipGetLastError());
    // The similarity kernels may be enqueued on a different stream than `s` (graph replay, a caller's stream):
    // the table must be complete before any of them can start.  Only runs after a template / geometry change.
    HIP_TRY(hipStreamSynchronize(s));
    c->foff_dirty = false;
    c->citems_dirty = true;
    return 0;
}

// per-slot records of the coarse pass (template record + threshold + first feature offsets): after any change of the
// active set, the thresholds, the templates or the geometry
int ensure_citems(sbm_ctx* c, hipStream_t s)
{
    const int n_active = (int)c->h_active.size();
    if (!c->citems_dirty || n_active == 0) return 0;
    if (c->rows[c->L - 1] <= 0) return 0; // no geometry yet: the first match call comes back here
    const int lc = c->L - 1, T = c->cfg.T[lc], W = c->cols[lc] / T, H = c->rows[lc] / T;
    if (int e = c->d_citems.ensure((size_t)n_active * sizeof(CoarseItem))) return e;
    if (int e = c->d_cfoff.ensure((size_t)n_active * 64 * 4)) return e;
    std::vector<int32_t> base((size_t)n_active);
    int64_t total = 0;
    for (int i = 0; i < n_active; ++i) {
        base[i] = (int32_t)total;
        total += c->h_tls[(size_t)c->h_active[i] * c->L + lc].nf;
    }
    if (total >= (int64_t)INT32_MAX) return fail(SBM_ERR_INVALID, "too many coarse-level features in the selection");
    if (int e = c->d_soff.ensure((size_t)std::max<int64_t>(total, 1) * 4)) return e;
    if (int e = c->d_soffbase.ensure((size_t)n_active * 4)) return e;
    HIP_TRY(hipMemcpyAsync(c->d_soffbase.p, base.data(), (size_t)n_active * 4, hipMemcpyHostToDevice, s));
    const int zero_off = (int)(7 * c->lm_stride[lc] + (int64_t)T * T * W * H);
    hipLaunchKernelGGL(k_prep_coarse_items, dim3((unsigned)((n_active + 63) / 64)), dim3(64), 0, s, c->d_active.as<int32_t>(), n_active,
                       c->d_tls.as<DevTL>(), c->L, lc, c->d_rawmin.as<int32_t>(), c->d_foff.as<int32_t>(), c->d_soffbase.as<int32_t>(), T, W, H,
                       zero_off, c->d_citems.as<CoarseItem>(), c->d_soff.as<int32_t>(), c->d_cfoff.as<int32_t>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s)); // consumers may run on another stream (as ensure_foff)
    c->citems_dirty = false;
    return 0;
}

// gradient stage + linear memories for every level; d_img0 may be external
// reset_count != null: the linear-memory launch also zeroes the per-frame counters and *reset_count
// (c->counters_fresh tells enqueue_coarse to skip its own k_reset launch).
//
// Row bands (build-sharded multi-GPU step, sbm_match_batch_device_banded): with bands.n > 1 the gradient stage of
// level l is launched only for the bands [bands.first, bands.first + bands.count) of bands.n equal row bands, each
// widened by band_halo(l) rows on either side -- the rows of level l whose fused cv::pyrDown output level l+1's band
// (itself widened) reads: halo(L-1) = 0, halo(l) = 2 * (halo(l+1) + 5) (7x7 Gaussian 3 + Sobel 1 + vote 1 rows of
// the next level's image on either side, two source rows each).  bands.between runs after the gradient launches and
// before the linear memories (the all-gather of the other ranks' bands).
struct Bands {
    int n = 1, first = 0, count = 1;
    int (*between)(sbm_ctx*, hipStream_t, int frames) = nullptr;
};

int band_halo(int L, int l)
{
    int e = 0;
    for (int k = L - 2; k >= l; --k) e = 2 * (e + 5);
    return e;
}

int check_bands(const sbm_ctx* c, int n_bands)
{
    if (n_bands < 1) return fail(SBM_ERR_INVALID, "n_bands must be >= 1");
    for (int l = 0; l < c->L; ++l)
        if (c->rows[l] % n_bands || ((c->rows[l] / n_bands) & 1))
            return fail(SBM_ERR_INVALID, "level %d: %d rows do not split into %d bands of an even number of rows", l, c->rows[l], n_bands);
    // The linear memories of a level must be built AFTER the exchange of its bands.  Only the one-launch builder runs
    // there (enqueue_pyramid: after bands->between); the generic per-level builder runs right behind the level's gradient
    // launch, i.e. on a map that still lacks the other ranks' rows.  Refuse such geometries instead of matching them wrong.
    for (int l = 0; l < c->L; ++l)
        if (!lm_rows_ok(c->d_quant[l].as<uint8_t>(), c->cols[l], c->cfg.T[l]))
            return fail(SBM_ERR_INVALID, "build-sharded match needs T in {4, 8} and 16-column-aligned levels (level %d: %d columns, T = %d)", l,
                        c->cols[l], c->cfg.T[l]);
    return 0;
}

// the context's own frames: level l's image (l >= 1: what level l-1's launch produced, fused cv::pyrDown), the retained level-0 source
FrameSource level_frames(const sbm_ctx* c, int l, int frames) { return packed_frames(c->d_img[l].p, c->rows[l], c->cols[l], c->channels, frames); }
FrameSource retained_frames(const sbm_ctx* c, int ch, int frames) { return packed_frames(c->d_src0.p, c->rows[0], c->cols[0], ch, frames); }

// The frames the sparse gradient launch of a call on `src` reads.  The caller's own where they are a fixed number of bytes apart
// and the streaming kernel takes their layout (it read callers' layouts, padded rows and frames included, before there was a
// sparse path): they stay valid until the call's work is done, and the call's source pass may then leave the retained copy
// unwritten (source_pass_retains).  Frames behind a table, a layout the kernel refuses and SBM_RETAIN_ALWAYS=1: the retained
// copy, which the source pass of such a call always stores.
FrameSource sparse_gradient_frames(const sbm_ctx* c, const FrameSource& src)
{
    const FrameSource kept = retained_frames(c, src.ch, src.frames);
    if (tuning().retain_always || src.kind != FRAMES_STRIDED || !src.base) return kept;
    if (!quantize_stream_rows(c, c->rows[0], c->cols[0], src, MaskSource{}, false)) return kept;
    return src;
}
bool reads_retained(const sbm_ctx* c, const FrameSource& sparse_src) { return sparse_src.base == c->d_src0.p; }

// A call's cursor down the pyramid: the caller's frames and masks at level 0, the context's own from level 1 on
struct PyramidCursor {
    FrameSource src;
    MaskSource mask;
};

// Rows [row_lo, row_hi) of level l's gradient stage, the one place it is launched from for a pyramid.  The first launch of a
// level l > 0 (first: the caller says so; further bands of the level find the cursor moved) moves the cursor down -- the mask
// resized from level l-1's, the image the one level l-1's launch produced.  A mask per frame stays a mask per frame down the
// pyramid (pyrDown(), line2Dup.cpp:439: level l's from level l-1's, frame by frame).
int enqueue_gradient_level(sbm_ctx* c, hipStream_t s, int l, bool first, PyramidCursor& cur, int row_lo, int row_hi)
{
    const int frames = cur.src.frames;
    if (l > 0 && first) {
        if (cur.mask.kind != MASK_NONE) {
            const int n = c->rows[l] * c->cols[l];
            const bool per_frame = masks_per_frame(cur.mask);
            if (per_frame && frames > c->mask_frames) return fail(SBM_ERR_STATE, "level %d holds %d masks, the batch has %d frames", l, c->mask_frames, frames);
            const int64_t dst_fs = per_frame ? (int64_t)n : 0;
            if (cur.mask.kind == MASK_TABLE) // level 0's masks are named by the caller's table; from here on they are the context's own
                SBM_LAUNCH(c, "k_resize_mask", k_resize_mask_ptrs, dim3(std::min((n + 255) / 256, 4096), frames), dim3(256), 0, s,
                           reinterpret_cast<const uint8_t* const*>(cur.mask.base), c->rows[l - 1], c->cols[l - 1], c->d_mask[l].as<uint8_t>(), c->rows[l],
                           c->cols[l], dst_fs);
            else
                SBM_LAUNCH(c, "k_resize_mask", k_resize_mask, dim3(std::min((n + 255) / 256, 4096), per_frame ? frames : 1), dim3(256), 0, s,
                           (const uint8_t*)cur.mask.base, c->rows[l - 1], c->cols[l - 1], c->d_mask[l].as<uint8_t>(), c->rows[l], c->cols[l],
                           kernel_mask_stride(cur.mask), dst_fs);
            HIP_TRY(hipGetLastError());
            cur.mask = strided_masks(c->d_mask[l].p, dst_fs);
        }
        cur.src = level_frames(c, l, frames);
    }
    QuantizeLaunch q;
    q.src = cur.src;
    q.mask = cur.mask;
    q.rows = c->rows[l], q.cols = c->cols[l];
    q.weak = c->cfg.weak_threshold;
    q.out = c->d_quant[l].as<uint8_t>();
    q.pyr = l + 1 < c->L ? c->d_img[l + 1].as<uint8_t>() : nullptr;
    q.row_lo = row_lo, q.row_hi = row_hi;
    return launch_quantize(c, s, q);
}

// What one call adds to the plan's inputs for a sparse level-0 gradient (PlanInputs::sparse_gradient ...): the knob and the
// retained buffer, whether both launches -- the source pass on the caller's frames, the later ones on the retained copy --
// take the streaming kernel, the mask, the bands (a one-band exchange reads the map too; level 0 launched already counts)
PlanInputs call_plan_inputs(const sbm_ctx* c, const FrameSource& src, const MaskSource& mask, const Bands* bands, bool level0_done)
{
    PlanInputs pin = plan_inputs(c);
    const int rows = c->rows[0], cols = c->cols[0], frames = src.frames;
    const int64_t fs = (int64_t)rows * cols * c->channels;
    pin.sparse_gradient = tuning().sparse_gradient && c->d_src0.p && fs < (int64_t)0x7ff00000 && (size_t)frames * (size_t)fs <= c->d_src0.cap;
    pin.l0_stream = pin.sparse_gradient && quantize_stream_rows(c, rows, cols, src, MaskSource{}, false) != 0 &&
                    quantize_stream_rows(c, rows, cols, retained_frames(c, c->channels, frames), MaskSource{}, false) != 0;
    pin.l0_mask = mask.kind != MASK_NONE;
    pin.banded = bands != nullptr || level0_done;
    pin.any_batch = frames > 1 && any_batch_ok(c);
    return pin;
}

// ... the plan of a match entry point then makes level 0's map sparsely
bool plans_sparse_gradient(const sbm_ctx* c, const FrameSource& src, const MaskSource& mask, const Bands* bands, bool level0_done)
{
    return plan_build(call_plan_inputs(c, src, mask, bands, level0_done), all_rows_ok(c), true).sparse_gradient;
}

// Every level of every frame of a batch in the forms of `plan` (LM_SPREAD or LM_PLANES8 per level), in one launch of
// k_build_lm_any: block ranges per level, coarsest first as in the one-launch builder, the frame as grid.y.  reset_count != null:
// the launch also zeroes the per-frame counters and the caller's counts (counters_fresh).
int launch_lm_any(sbm_ctx* c, hipStream_t s, const BuildPlan& plan, int frames, int32_t* reset_count)
{
    LmaArgs a;
    memset(&a, 0, sizeof a);
    int64_t blocks = 0;
    int smem = 0;
    for (int l = c->L - 1; l >= 0; --l) {
        const int T = c->cfg.T[l], W = c->cols[l] / T, H = c->rows[l] / T;
        const LmForm f = plan.form[l];
        if (T > LMA_MAX_T || (f != LM_SPREAD && f != LM_PLANES8) || (f == LM_SPREAD && !c->d_lmc[l].p))
            return fail(SBM_ERR_STATE, "level %d (T = %d, form %d) is not one the batched any-stride builder makes", l, T, (int)f);
        const LmaShape sh = lma_shape(T);
        const int64_t stride = c->lm_stride[l];
        a.lv[a.n_levels] = LmaLevel{c->d_quant[l].as<uint8_t>(), f == LM_SPREAD ? c->d_lmc[l].as<uint8_t>() : c->d_lm[l].as<uint8_t>(), stride,
                                    (int64_t)c->rows[l] * c->cols[l], (f == LM_SPREAD ? 1 : 8) * stride, c->rows[l], c->cols[l], W, H, T,
                                    sh.cells, sh.grows, (int32_t)f};
        a.block_begin[a.n_levels++] = (int32_t)blocks;
        blocks += lma_level_blocks(W, H, sh);
        smem = std::max(smem, lma_lds_bytes(T, sh.cells, sh.grows));
    }
    if (blocks >= (int64_t)INT32_MAX) return fail(SBM_ERR_INVALID, "pyramid too large for one linear-memory launch");
    if (reset_count) {
        a.counters = c->d_counters.as<int32_t>();
        a.out_count = reset_count;
        c->counters_fresh = true;
    }
    SBM_LAUNCH(c, "k_build_lm", k_build_lm_any, dim3((unsigned)blocks, frames), dim3(LMA_THREADS), (size_t)smem, s, a);
    HIP_TRY(hipGetLastError());
    for (int l = 0; l < c->L; ++l) c->rec.note_level_build(l, plan.form[l], 2);
    return 0;
}

// src0 / mask0: level 0's frames and masks, the caller's or the context's own
int enqueue_pyramid(sbm_ctx* c, hipStream_t s, const FrameSource& src0, const MaskSource& mask0, int32_t* reset_count = nullptr,
                    const Bands* bands = nullptr, bool level0_gradient_done = false)
{
    PyramidCursor cur{src0, mask0};
    const int frames = src0.frames;
    c->rec.begin_build(frames);
    const bool all_rows = all_rows_ok(c);
    c->counters_fresh = false;
    c->call_counted = false;
    // A match entry point (it passes reset_count and has set the threshold already) whose coarse pass will run on bit planes
    // builds the coarsest level as bit planes ONLY, inside the one linear-memory launch, and its T = 4 strip levels as bit strips.
    // The stage entry points keep the 8 response planes there (the bit planes are then packed from them on demand).
    const PlanInputs pin = call_plan_inputs(c, src0, mask0, bands, level0_gradient_done);
    const BuildPlan plan = plan_build(pin, all_rows, reset_count != nullptr);
    // off the one-launch builder's grid a batch takes k_build_lm_any, which is sized for strides up to LMA_MAX_T
    if (!all_rows && frames > 1 && !pin.any_batch) {
        for (int l = 0; l < c->L; ++l)
            if (c->cfg.T[l] > LMA_MAX_T)
                return fail(SBM_ERR_INVALID, "batched match: level %d has T = %d, and a pyramid with a stride other than 4 or 8 or a level that is not "
                            "16-column-aligned batches up to T = %d only", l, c->cfg.T[l], LMA_MAX_T);
        return fail(SBM_ERR_STATE, "batched match: no linear-memory builder for this pyramid");
    }
    // (the linear memories of a level right behind its gradient launch -- two launches per batch, the orientation map still
    // in the caches -- measure the same as one launch for all levels at the end: tools/r03_lm_early.sh)
    for (int l = 0; l < c->L; ++l) {
        const int nb = (l == 0 && level0_gradient_done) ? 0 : (bands && bands->n > 1 ? bands->count : 1);
        for (int b = 0; b < nb; ++b) {
            int lo = 0, hi = c->rows[l];
            if (bands && bands->n > 1) {
                const int br = c->rows[l] / bands->n, e = band_halo(c->L, l);
                lo = std::max(0, (bands->first + b) * br - e);
                hi = std::min(c->rows[l], (bands->first + b + 1) * br + e);
            }
            if (l == 0 && plan.sparse_gradient) {
                // the source pass: level 1's image and the retained copy; the map waits for the coarse candidates (enqueue_sparse_strips)
                QSForm form{QS_SOURCE, c->d_src0.as<uint8_t>(), (int64_t)c->rows[0] * c->cols[0] * c->channels, nullptr, 0, 0, 0, 0};
                // The copy is stored while no later call is enqueued behind this one -- where this call's own sparse launch reads
                // the caller's frames.  Where it reads the copy, the counters it is given are the word that is always 0.
                c->sparse_src = sparse_gradient_frames(c, src0);
                uint32_t* const w = c->d_call.as<uint32_t>();
                const bool follows = !reads_retained(c, c->sparse_src) && c->d_enqueued;
                form.call_enqueued = follows ? w + CALL_SEEN : w + CALL_ZERO; // (the host's count as a launch before this one read it)
                form.call_executed = follows ? w + CALL_EXECUTED : w + CALL_ZERO;
                form.call_note = w + CALL_NOTE;
                QuantizeLaunch q;
                q.src = src0;
                q.rows = c->rows[0], q.cols = c->cols[0];
                q.weak = c->cfg.weak_threshold;
                q.out = c->d_quant[0].as<uint8_t>();
                q.pyr = c->d_img[1].as<uint8_t>();
                q.form = &form;
                if (int e = launch_quantize(c, s, q)) return e;
                continue;
            }
            if (int e = enqueue_gradient_level(c, s, l, b == 0, cur, lo, hi)) return e;
        }
        if (!all_rows && !pin.any_batch)
            if (int e = launch_build_lm(c, s, l)) return e;
    }
    if (bands && bands->between)
        if (int e = bands->between(c, s, frames)) return e;
    if (all_rows) {
        // every level's linear memories in one launch (block ranges coarsest level first: its blocks -- T * 8 / 4 stores per
        // lane -- are the long ones, and a launch that dispatches its long blocks last ends with a few of them running alone),
        // which also zeroes the per-frame counters and *reset_count
        // A level planned as sparse bit strips has no share in it: its tiles are built behind the coarse pass (enqueue_sparse_strips);
        // this launch clears their flags.
        LmArgs a;
        memset(&a, 0, sizeof a);
        int blocks = 0;
        for (int l = c->L - 1, n = 0; l >= 0; --l) {
            if (plan.form[l] == LM_BIT_STRIPS_SPARSE) continue;
            a.lv[a.n_levels++] = lm_level_args(c, l, plan.form[l], frames, blocks, &n);
            blocks += n;
        }
        if (reset_count) {
            a.counters = c->d_counters.as<int32_t>();
            a.out_count = reset_count;
            c->counters_fresh = true;
            a.call_words = c->d_call.as<uint32_t>(); // a match call: counted where its counters are reset (enqueue_match)
            a.call_enqueued = c->d_enqueued;         // (null: nothing is read, every call keeps its copy)
            c->call_counted = true;
            if (plan.form[0] == LM_BIT_STRIPS_SPARSE) {
                a.clear_tiles = c->d_tiles.as<uint8_t>();
                a.n_tiles = refine_tile_count(c->cols[0] / c->cfg.T[0], c->rows[0] / c->cfg.T[0]);
                a.clear_rects = c->d_rects.as<int32_t>(); // (null without the record)
                a.n_bands = refine_band_count(c->rows[0]);
                a.clear_items = c->d_items.as<int32_t>(); // (null without the lists)
                a.items_stride = refine_list_stride(c->items_cap);
            }
        }
        SBM_LAUNCH(c, "k_build_lm", k_build_lm_rows, dim3(blocks, frames), dim3(256), 0, s, a);
        HIP_TRY(hipGetLastError());
        for (int i = 0; i < a.n_levels; ++i) { // (a.lv[] is coarsest first and skips a sparse level 0)
            const int l = c->L - 1 - i;
            c->rec.note_level_build(l, plan.form[l], 1, a.lv[i].split, a.lv[i].allty);
        }
    } else if (pin.any_batch) {
        if (int e = launch_lm_any(c, s, plan, frames, reset_count)) return e;
    }
    if (plan.pack_spread) { // the spread plane is row-major, the flat order of the byte planes
        const int l = c->L - 1;
        const int n_dwords = (int)(((int64_t)c->rows[l] * c->cols[l] + 31) / 32);
        SBM_LAUNCH(c, "k_pack_bitplanes", k_pack_bitplanes_spread, dim3((n_dwords + 255) / 256, frames), dim3(256), 0, s, c->d_lmc[l].as<uint8_t>(),
                   c->lm_stride[l], c->lm_stride[l], c->d_blm.as<uint32_t>(), (int64_t)(2 * c->lm_stride[l]) / 4, n_dwords);
        HIP_TRY(hipGetLastError());
        c->rec.level_build[l].packed = 1;
    }
    record_build(c->rec.forms, c->L, plan);
    c->rec.levels_valid = c->L;
    c->rec.map0_whole = !plan.sparse_gradient;
    if (plan.sparse_gradient) c->rec.src0_ch = c->channels;
    return 0;
}

// d_quant[0] whole in every frame of the last batch, for a reader other than the sparse call's own strip builder: the ordinary
// gradient launch on the retained source.  On the reader's stream, outside any capture.
int ensure_level0_map(sbm_ctx* c, hipStream_t s)
{
    if (c->rec.map0_whole || c->rec.levels_valid < 1) return 0;
    const int rows = c->rows[0], cols = c->cols[0], ch = c->rec.src0_ch;
    if (!c->d_src0.p || (size_t)c->rec.last_frames * rows * cols * ch > c->d_src0.cap) return fail(SBM_ERR_STATE, "level 0's source is not retained");
    // The copy this reads is the one of the last match call enqueued, which stores it unless a later call is enqueued before its
    // source pass runs (source_pass_retains).  Wait for that call here: it then ran as the last one enqueued and has stored its
    // copy, whatever the host enqueues behind this reader.  The context's own event stands for the call: the caller's stream may
    // be gone by now.
    if (!c->call_recorded || hipEventSynchronize(c->ev_call) != hipSuccess) {
        (void)hipGetLastError();
        HIP_TRY(hipDeviceSynchronize());
    }
    QuantizeLaunch q;
    q.src = retained_frames(c, ch, c->rec.last_frames);
    q.rows = rows, q.cols = cols;
    q.weak = c->cfg.weak_threshold;
    q.out = c->d_quant[0].as<uint8_t>();
    if (int e = launch_quantize(c, s, q)) return e;
    c->rec.map0_whole = true;
    return 0;
}

// The host-memory entry points (sbm_match, sbm_match_batch_host*, sbm_build_pyramid, sbm_set_quantized,
// sbm_match_templates, sbm_get_quantized) reuse the context's buffers on its own stream, which does not wait for a caller's
// stream: a device entry point enqueued there just before may still be writing the same orientation maps, linear memories
// and counters.  Only after such a call, wait for the device once; contexts that never see a caller's stream pay nothing.
int order_after_caller_work(sbm_ctx* c)
{
    if (!c->caller_work) return 0;
    HIP_TRY(hipDeviceSynchronize());
    c->caller_work = false;
    return 0;
}

// the stream a device entry point launches on: the caller's (remembered for order_after_caller_work), else the context's
hipStream_t launch_stream(sbm_ctx* c, void* stream)
{
    if (stream && (hipStream_t)stream != c->stream) c->caller_work = true;
    return stream ? (hipStream_t)stream : c->stream;
}

// the template tables of this threshold are not resident yet: frames in flight may still read the ones about to change
bool templates_dirty(const sbm_ctx* c, float threshold) { return !c->have_thr || memcmp(&threshold, &c->thr_cached, 4) != 0 || c->foff_dirty; }

// ... or the geometry, the batch size or the pyramid are about to change
bool match_dirty(const sbm_ctx* c, int rows, int cols, int channels, int frames, float threshold)
{
    return !(c->channels == channels && c->rows[0] == rows && c->cols[0] == cols && c->rec.levels_valid == c->L && frames <= c->batch) ||
           templates_dirty(c, threshold);
}

// host-side preparation of the template loop: validation, integer thresholds, feature offsets.
// May synchronise (only when something changed); never called inside a stream capture.
// The tables are (re)built on the CONTEXT's stream and that stream is synchronised by the host, whatever stream the
// consumers will run on: the caller's stream is neither waited on nor given work here (ADVICE round 2: a host wait on
// the caller's stream fails while that stream is being captured).  Nothing is enqueued when nothing changed.
int prepare_templates(sbm_ctx* c, float threshold, int64_t cap)
{
    if (c->n_templates == 0) return fail(SBM_ERR_STATE, "no templates uploaded");
    if (cap < 0 || cap > INT32_MAX) return fail(SBM_ERR_INVALID, "bad output capacity");
    if (int e = ensure_thresholds(c, threshold, c->stream)) return e;
    if (int e = ensure_foff(c, c->stream)) return e;
    return ensure_citems(c, c->stream);
}

// One match call as every entry point describes it: frames of rows x cols x ch pixels, frame_stride bytes apart, against the
// active templates; per frame up to cap records into out and a {n_matches, overflow} pair into counts (device memory)
struct MatchCall {
    FrameSource src;
    MaskSource mask;
    int rows, cols;
    float thr;
    sbm_match_rec* out;
    int64_t cap;
    int32_t* counts;
};

int check_stride(int stride, int cols, int ch)
{
    return stride < cols * ch ? fail(SBM_ERR_INVALID, "stride %d < cols*channels", stride) : 0;
}

int check_match_call(const sbm_ctx* c, const MatchCall& m)
{
    if (!c || !m.src.base || !m.out || !m.counts) return fail(SBM_ERR_INVALID, "null argument");
    if (m.src.frames < 1) return fail(SBM_ERR_INVALID, "n_frames must be >= 1");
    if (int e = check_stride(m.src.stride, m.cols, m.src.ch)) return e;
    // (one frame: the frame stride is not read)
    if (m.src.frames > 1 && m.src.frame_stride < (int64_t)m.src.stride * m.rows) return fail(SBM_ERR_INVALID, "frame_stride smaller than one frame");
    if (m.mask.kind == MASK_STRIDED && m.mask.stride < (int64_t)m.rows * m.cols) return fail(SBM_ERR_INVALID, "mask_stride smaller than one mask");
    return 0;
}

// The prologue of a match call, before anything of it is enqueued, once the device is set and the stream chosen.
// Whatever the call is about to change (geometry, batch size, pyramid, template tables; also_dirty: anything else the
// caller knows of) may still be read by frames in flight, so the device is waited for first; every later state change
// of the call happens here too (it may synchronise), so that the launches can be replayed as a graph.
int settle_match_state(sbm_ctx* c, const MatchCall& m, const Bands* bands, bool also_dirty)
{
    const bool frame_masks = masks_per_frame(m.mask);
    if (match_dirty(c, m.rows, m.cols, m.src.ch, m.src.frames, m.thr) || also_dirty || (frame_masks && m.src.frames > c->mask_frames)) HIP_TRY(hipDeviceSynchronize());
    if (int e = ensure_geometry(c, m.rows, m.cols, m.src.ch, m.src.frames, frame_masks)) return e;
    if (bands)
        if (int e = check_bands(c, bands->n)) return e;
    if (c->profiling && !c->profiling_keep) c->clear_timings();
    return prepare_templates(c, m.thr, m.cap);
}

// ... of a device entry point: on the caller's stream or the context's
int begin_match(sbm_ctx* c, void* stream, const MatchCall& m, hipStream_t* s, const Bands* bands = nullptr)
{
    HIP_TRY(hipSetDevice(c->cfg.device_id));
    *s = launch_stream(c, stream);
    return settle_match_state(c, m, bands, false);
}

// ... of a host entry point: on the context's own stream, behind whatever a device entry point left on a caller's
int begin_host_match(sbm_ctx* c, const MatchCall& m, bool also_dirty = false)
{
    HIP_TRY(hipSetDevice(c->cfg.device_id));
    if (int e = order_after_caller_work(c)) return e;
    return settle_match_state(c, m, nullptr, also_dirty);
}

// the coarsest level's bit planes (of `frames` frames) packed from its 8 response planes
int pack_bitplanes(sbm_ctx* c, hipStream_t s, int frames)
{
    const int lc = c->L - 1, T = c->cfg.T[lc], W = c->cols[lc] / T, H = c->rows[lc] / T;
    if (!c->rec.forms[lc].planes8) return fail(SBM_ERR_STATE, "linear memories of level %d are not built", lc);
    const int n_dwords = (int)(((int64_t)T * T * W * H + 31) / 32);
    SBM_LAUNCH(c, "k_pack_bitplanes", k_pack_bitplanes, dim3((n_dwords + 255) / 256, 8, frames), dim3(256), 0, s, c->d_lm[lc].as<uint8_t>(),
               c->lm_stride[lc], (int64_t)8 * c->lm_stride[lc], c->d_blm.as<uint32_t>(), (int64_t)(2 * c->lm_stride[lc]) / 4, n_dwords);
    HIP_TRY(hipGetLastError());
    record_pack(c->rec.forms[lc]);
    c->rec.level_build[lc].packed = 2;
    return 0;
}

// What the coarse pass of the current threshold reads, made current outside any capture: the bit planes packed from the
// response planes (stage entry points: the pyramid was set level by level), or the response planes rebuilt after a
// bits-only build when a byte kernel is asked for.
int ensure_coarse_planes(sbm_ctx* c, hipStream_t s)
{
    if (!coarse_on_bits(c)) return ensure_full_lm(c, c->L - 1, s);
    return c->rec.forms[c->L - 1].bit_planes ? 0 : pack_bitplanes(c, s, 1);
}

// positions of the coarsest level's W x H grid a template is scored at (the host's side of the device's template_positions)
int host_template_npos(const DevTL& tl, int T, int W, int H)
{
    const int wf = (tl.width - 1) / T + 1, hf = (tl.height - 1) / T + 1;
    return (H - hf) * W + (W - wf) + 1;
}

// h_fxy after an upload that left the features on the device: one copy of d_fxy, at the first call that counts features on
// the host (sbm_partition_templates, sbm_coarse_bytes).  The upload ended with a device-wide wait, so d_fxy is complete.
int ensure_host_fxy(sbm_ctx* c)
{
    if (c->h_fxy_valid) return 0;
    HIP_TRY(hipSetDevice(c->cfg.device_id));
    std::vector<uint32_t> fxy((size_t)c->n_features);
    if (!fxy.empty()) HIP_TRY(hipMemcpy(fxy.data(), c->d_fxy.p, fxy.size() * 4, hipMemcpyDeviceToHost));
    c->h_fxy.swap(fxy);
    c->h_fxy_valid = true;
    return 0;
}

// features of a template level that lie inside a rows x cols level: the ones its coarse pass adds (after ensure_host_fxy)
int64_t features_in_bounds(const sbm_ctx* c, const DevTL& tl, int rows, int cols)
{
    int64_t n = 0;
    for (int k = 0; k < tl.nf; ++k) {
        const uint32_t xy = c->h_fxy[tl.feat_off + k];
        if ((int)(xy & 0xffff) < cols && (int)(xy >> 16) < rows) ++n;
    }
    return n;
}

// coarse pass over the active templates (reset + k_similarity_coarse; single-level pyramids emit here)
// clear_tiles: where its own k_reset runs, that also clears frame 0's refinement-tile flags (a sparse call's retry)
int enqueue_coarse(sbm_ctx* c, hipStream_t s, sbm_match_rec* d_out, int64_t cap, int32_t* d_count, int frames = 1, bool clear_tiles = false)
{
    const int L = c->L, lc = L - 1;
    int32_t* counters = c->d_counters.as<int32_t>();
    if (!c->counters_fresh && frames > 1) return fail(SBM_ERR_STATE, "batched template loop without a batched pyramid");
    if (!c->counters_fresh)
        hipLaunchKernelGGL(k_reset, dim3(1), dim3(64), 0, s, counters, d_count, clear_tiles ? c->d_tiles.as<uint8_t>() : (uint8_t*)nullptr,
                           clear_tiles ? refine_tile_count(c->cols[0] / c->cfg.T[0], c->rows[0] / c->cfg.T[0]) : 0,
                           clear_tiles ? c->d_rects.as<int32_t>() : (int32_t*)nullptr, clear_tiles ? refine_band_count(c->rows[0]) : 0,
                           clear_tiles ? c->d_items.as<int32_t>() : (int32_t*)nullptr);
    c->counters_fresh = false;
    const int n_active = (int)c->h_active.size();
    if (n_active > 0) {
        const int T = c->cfg.T[lc], W = c->cols[lc] / T, H = c->rows[lc] / T;
        int chunks = (W * H + COARSE_POS_PER_BLOCK - 1) / COARSE_POS_PER_BLOCK;
        // chunks of `per` positions that cover the positions some template reaches
        auto coarse_chunks = [W, H](int npos, int per) { return std::max(1, (std::min(std::max(npos, 0), W * H) + per - 1) / per); };
        int bits_max_npos = 0;
        if (c->thr_cached >= 0.f) {
            // every raw_min is >= 1, so positions past a template's span (score 0) are never candidates:
            // launch only the chunks some template reaches; a multiple of 8 of them lets the kernel give
            // each XCD a contiguous, equally loaded range of chunks (its L2 then holds one slice of the
            // linear memories)
            int max_npos = 0;
            for (int32_t t : c->h_active) max_npos = std::max(max_npos, host_template_npos(c->h_tls[(size_t)t * L + lc], T, W, H));
            bits_max_npos = max_npos;
            int need = coarse_chunks(max_npos, COARSE_POS_PER_BLOCK);
            if (need >= 8) need = (need + 7) / 8 * 8;
            chunks = std::min(need, (chunks + 7) / 8 * 8);
        }
        // Round 4: the bit-plane kernel (sbm_coarse_bits.h) whenever every raw_min is >= 1 (threshold >= 0: positions past
        // a template's span are never candidates); SBM_COARSE / sbm_set_coarse_mode pick a byte kernel instead.
        const PlanInputs pin = plan_inputs(c);
        const bool bits = coarse_on_bits(pin);
        if (!bits && !c->rec.forms[lc].planes8) {
            // a byte kernel after a match call that built the bit planes only (the stage entry point with a threshold < 0)
            if (frames > 1) return fail(SBM_ERR_STATE, "the coarsest level's response planes are not built");
            if (int e = ensure_full_lm(c, lc, s)) return e;
        }
        int max_nf = 0, bits_dw = 1;
        if (bits) {
            for (int32_t t : c->h_active) max_nf = std::max(max_nf, c->h_tls[(size_t)t * L + lc].nf);
            if (coarse_packs_planes(pin, c->rec.forms[lc], false))
                if (int e = pack_bitplanes(c, s, frames)) return e;
            chunks = coarse_chunks(bits_max_npos, CB_POS);
            // Two dwords (64 positions) per lane -- half as many, twice as long work items -- when the one-dword items would
            // not all be resident at once (8 waves per SIMD): a second round of waves starts only when the first ends, and the
            // launch then takes two "longest waves" instead of one.  SBM_BITS_DW=1|2 forces either.
            bits_dw = tuning().bits_dw ? tuning().bits_dw
                                       : (max_nf < 1024 && (int64_t)chunks * n_active * frames > (int64_t)c->n_simd * 8 ? 2 : 1);
            if (bits_dw == 2) chunks = coarse_chunks(bits_max_npos, 2 * CB_POS);
        }
        // the latency form (eight waves per item, no pruning) for launches of a few hundred items: one frame, a few hundred templates
        const bool bits_block = bits && (tuning().bits_block < 0 ? (int64_t)chunks * n_active * frames <= 2048 : tuning().bits_block != 0);
        for (int first = 0; first < n_active; first += 65535) {
            const int cnt = std::min(65535, n_active - first);
            if (bits_block) {
                const int chunks1 = coarse_chunks(bits_max_npos, CB_POS);
#define SBM_COARSE_BITS_BLOCK(P_)                                                                                                    \
                c->rec.note_coarse_form(4, P_, false, 0);                                                                                 \
                SBM_LAUNCH(c, "k_similarity_coarse", (k_similarity_coarse_bits_block<P_>), dim3(chunks1, cnt, frames), dim3(512), 0, s,   \
                           c->d_blm.as<uint32_t>(), c->lm_stride[lc], T, W, H, L, lc, c->d_tls.as<DevTL>(), c->d_soff.as<int32_t>(),   \
                           c->d_citems.as<CoarseItem>() + first, cnt, c->d_rawkeep.as<int32_t>(), c->d_class.as<int32_t>(),             \
                           c->d_tid.as<int32_t>(), c->d_cands.as<Cand>(), counters, (int)c->cand_cap, (int64_t)(2 * c->lm_stride[lc]) / 4)
                if (max_nf < 128) { SBM_COARSE_BITS_BLOCK(7); }
                else if (max_nf < 1024) { SBM_COARSE_BITS_BLOCK(10); }
                else { SBM_COARSE_BITS_BLOCK(13); }
#undef SBM_COARSE_BITS_BLOCK
                continue;
            }
            if (bits) {
#define SBM_COARSE_BITS(P_)                                                                                                          \
                if (tuning().bits_wide < 0 ? max_nf >= 64 : tuning().bits_wide != 0) SBM_COARSE_BITS_W(P_, true); else SBM_COARSE_BITS_W(P_, false)
#define SBM_COARSE_BITS_W(P_, W_)                                                                                                    \
                if (bits_dw == 2) SBM_COARSE_BITS_D(P_, W_, 2); else SBM_COARSE_BITS_D(P_, W_, 1)
#define SBM_COARSE_BITS_D(P_, W_, D_)                                                                                                \
                do {                                                                                                                  \
                c->rec.note_coarse_form(3, P_, W_, D_);                                                                                   \
                SBM_LAUNCH(c, "k_similarity_coarse", (k_similarity_coarse_bits<P_, W_, D_>), dim3(chunks, (cnt + 3) / 4, frames), dim3(256), 0, s, \
                           c->d_blm.as<uint32_t>(), c->lm_stride[lc], T, W, H, L, lc, c->d_tls.as<DevTL>(), c->d_soff.as<int32_t>(),   \
                           c->d_citems.as<CoarseItem>() + first, c->d_cfoff.as<int32_t>() + (size_t)first * 64, cnt,                     \
                           c->d_rawkeep.as<int32_t>(), c->d_class.as<int32_t>(), c->d_tid.as<int32_t>(), c->d_cands.as<Cand>(), counters, \
                           (int)c->cand_cap, (int64_t)(2 * c->lm_stride[lc]) / 4);                                                      \
                } while (0)
                if (max_nf < 128) SBM_COARSE_BITS(7);
                else if (max_nf < 1024) SBM_COARSE_BITS(10);
                else SBM_COARSE_BITS_W(13, true); // thousands of features: always the wide batches, one dword per lane
#undef SBM_COARSE_BITS
#undef SBM_COARSE_BITS_W
#undef SBM_COARSE_BITS_D
                continue;
            }
            // large launches: one wave per (chunk, template, frame); small ones (a single frame with a few hundred
            // templates): four waves share an item's features so that enough loads are in flight
            const bool per_wave = c->coarse_mode == 2 || (c->coarse_mode != 1 && (int64_t)chunks * cnt * frames >= 8192);
            c->rec.note_coarse_form(per_wave ? 2 : 1, 0, false, 0);
            if (per_wave)
                SBM_LAUNCH(c, "k_similarity_coarse", k_similarity_coarse_wave, dim3(chunks, (cnt + 3) / 4, frames), dim3(256), 0, s,
                           c->d_lm[lc].as<uint8_t>(), c->lm_stride[lc], c->rows[lc], c->cols[lc], T, W, H, L, lc, c->d_tls.as<DevTL>(),
                           c->d_soff.as<int32_t>(), c->d_citems.as<CoarseItem>() + first, c->d_cfoff.as<int32_t>() + (size_t)first * 64, cnt,
                           c->d_rawkeep.as<int32_t>(), c->d_class.as<int32_t>(), c->d_tid.as<int32_t>(),
                           c->d_cands.as<Cand>(), counters, (int)c->cand_cap, (int64_t)8 * c->lm_stride[lc]);
            else
                SBM_LAUNCH(c, "k_similarity_coarse", k_similarity_coarse, dim3(chunks, cnt, frames), dim3(256), 0, s, c->d_lm[lc].as<uint8_t>(),
                           c->lm_stride[lc], c->rows[lc], c->cols[lc], T, W, H, L, lc, c->d_tls.as<DevTL>(), c->d_fxy.as<uint32_t>(),
                           c->d_foff.as<int32_t>(), c->d_active.as<int32_t>() + first, c->d_rawmin.as<int32_t>(),
                           c->d_rawkeep.as<int32_t>(), c->d_class.as<int32_t>(), c->d_tid.as<int32_t>(),
                           c->d_cands.as<Cand>(), counters, (int)c->cand_cap, (int64_t)8 * c->lm_stride[lc]);
        }
        HIP_TRY(hipGetLastError());
    }
    if (L == 1) {
        SBM_LAUNCH(c, "k_emit_coarse", k_emit_coarse, dim3(256, frames), dim3(256), 0, s, c->d_cands.as<Cand>(), counters, (int)c->cand_cap,
                           c->d_tls.as<DevTL>(), L, lc, c->d_class.as<int32_t>(), c->d_tid.as<int32_t>(), d_out, d_count,
                           (int)cap, c->mirror_out, c->mirror_count);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

// refinement passes, finest level last (emits the match records)
// sparse0: level 0's bit strips were built for this call's candidates alone (enqueue_sparse_strips); the record calls nothing current
int enqueue_local(sbm_ctx* c, hipStream_t s, sbm_match_rec* d_out, int64_t cap, int32_t* d_count, int frames = 1, bool raised = false,
                  bool sparse0 = false)
{
    const int L = c->L;
    int32_t* counters = c->d_counters.as<int32_t>();
    for (int l = L - 2; l >= 0; --l) {
        const int T = c->cfg.T[l], W = c->cols[l] / T, H = c->rows[l] / T;
        // candidate slots per frame (a workgroup loops over the candidates slot, slot + grid, ...): 512 finishes a launch
        // that runs alone soonest on candidate-heavy frames (36 against 39.5 us on 16 tiled frames); with several batches in
        // flight (sbm_set_pipeline_depth) the idle workgroups of a large grid only take dispatch slots from the other
        // batches' kernels: 128 (pipelined step 115.5 -> 114.5 us on the scene frame, 148 -> 145.5 on the tiled one)
        const int local_grid_env = tuning().local_grid;
        const int local_grid = local_grid_env ? local_grid_env : (c->pipeline_depth >= 2 ? 128 : 512);
        // the kernel walks the candidates of up to 64 frames as one frame-major list: grid = (workgroups, 64-frame groups)
        // which candidate a workgroup takes (k_similarity_local's ORDER): one frame-major list once the batch's planes
        // of this level no longer fit the eight L2s together
        const int64_t planes = (int64_t)frames * c->rows[l] * c->cols[l];
        int order = c->local_order >= 0 ? c->local_order : (planes > (32 << 20) ? 2 : 0);
        const dim3 local_dim = order == 2 ? dim3((unsigned)(std::min(frames, 64) * local_grid), (unsigned)((frames + 63) / 64))
                                          : dim3(frames, local_grid);
        const LmForm reads = l == 0 && sparse0 ? LM_BIT_STRIPS : refine_reads(c->rec.forms[l]);
        if (reads == LM_NONE) return fail(SBM_ERR_STATE, "linear memories of level %d are not built", l);
        const int local_waves = tuning().local_waves; // 4 or 16
        const bool small_blocks = local_waves ? local_waves == 4 : frames >= 4;
#define SBM_LOCAL(COMPACT_, LM_, FS_)                                                                                               \
        if (small_blocks) SBM_LOCAL_LW(COMPACT_, LM_, FS_, 4); else SBM_LOCAL_LW(COMPACT_, LM_, FS_, LOCAL_WAVES)
#define SBM_LOCAL_LW(COMPACT_, LM_, FS_, LW_)                                                                                       \
        if (order == 2) SBM_LOCAL_O(COMPACT_, LM_, FS_, LW_, 2); else SBM_LOCAL_O(COMPACT_, LM_, FS_, LW_, 0)
#define SBM_LOCAL_O(COMPACT_, LM_, FS_, LW_, ORDER_)                                                                               \
        if ((COMPACT_) == 2 && T == 8) SBM_LOCAL_T(COMPACT_, LM_, FS_, LW_, ORDER_, (COMPACT_) == 2); else SBM_LOCAL_T(COMPACT_, LM_, FS_, LW_, ORDER_, false)
#define SBM_LOCAL_T(COMPACT_, LM_, FS_, LW_, ORDER_, T8_)                                                                          \
        SBM_LAUNCH(c, "k_similarity_local", (k_similarity_local<COMPACT_, LW_, ORDER_, T8_>), local_dim, dim3(64 * LW_), 0, s, LM_,    \
                   c->lm_stride[l], c->rows[l], c->cols[l], T, W, H, L, l, c->d_tls.as<DevTL>(),                                   \
                   (COMPACT_) == 2 ? c->d_fxy_s.as<uint32_t>() : c->d_fxy.as<uint32_t>(),                                          \
                   c->d_foff.as<int32_t>(), c->d_rawkeep.as<int32_t>(), c->d_class.as<int32_t>(), c->d_tid.as<int32_t>(),          \
                   c->d_cands.as<Cand>(), counters, (int)c->cand_cap, l == 0 ? 1 : 0, d_out, d_count, (int)cap, c->mirror_out,     \
                   c->mirror_count, (c->profiling ? 1 : 0) | (raised ? 2 : 0), (int64_t)(FS_) * c->lm_stride[l],                                       \
                   (COMPACT_) == 2 ? c->d_flabel_s.as<uint8_t>() : c->d_flabel.as<uint8_t>(), c->d_fcls.as<uint16_t>(), frames)
        if (reads == LM_BIT_STRIPS) {
            // bit strips: one wave per candidate (four times the slots of the four-wave byte form)
            const int slots = local_grid_env ? local_grid_env : 4 * local_grid;
            // batches whose strips exceed the L2s: the slot order with every XCD taking its frames one after the other (flag 4)
            // instead of the frame-major list, when the frames divide among the XCDs
            const bool xcd_seq = order == 2 && c->local_order < 0 && (frames & 7) == 0;
            if (xcd_seq) order = 0;
            const dim3 bits_dim = order == 2 ? dim3((unsigned)(std::min(frames, 64) * slots), (unsigned)((frames + 63) / 64)) : dim3(frames, slots);
#define SBM_LOCAL_BITS(ORDER_)                                                                                                      \
            SBM_LAUNCH(c, "k_similarity_local", (k_similarity_local_bits<ORDER_>), bits_dim, dim3(64), 0, s, c->d_lbits[l].as<uint8_t>(),  \
                       c->lm_stride[l], c->rows[l], c->cols[l], T, W, H, L, l, c->d_tls.as<DevTL>(), c->d_fxy.as<uint32_t>(),       \
                       c->d_foff.as<int32_t>(), c->d_rawkeep.as<int32_t>(), c->d_class.as<int32_t>(), c->d_tid.as<int32_t>(),       \
                       c->d_cands.as<Cand>(), counters, (int)c->cand_cap, l == 0 ? 1 : 0, d_out, d_count, (int)cap, c->mirror_out,  \
                       c->mirror_count, (c->profiling ? 1 : 0) | (raised ? 2 : 0) | (xcd_seq ? 4 : 0), lbits_frame_bytes(c, l),    \
                       c->d_flabel.as<uint8_t>(), c->d_fcls.as<uint16_t>(), frames)
            if (order == 2) SBM_LOCAL_BITS(2);
            else SBM_LOCAL_BITS(0);
#undef SBM_LOCAL_BITS
            c->rec.note_refine_form(l, reads, 1, order, false, l == 0 && sparse0, slots);
        }
        else if (reads == LM_SPREAD_STRIP) { SBM_LOCAL(2, c->d_lmc[l].as<uint8_t>(), 1); }
        else if (reads == LM_SPREAD) { SBM_LOCAL(1, c->d_lmc[l].as<uint8_t>(), 1); }
        else { SBM_LOCAL(0, c->d_lm[l].as<uint8_t>(), 8); }
#undef SBM_LOCAL
#undef SBM_LOCAL_LW
#undef SBM_LOCAL_O
#undef SBM_LOCAL_T
        if (reads != LM_BIT_STRIPS) c->rec.note_refine_form(l, reads, small_blocks ? 4 : LOCAL_WAVES, order, reads == LM_SPREAD_STRIP && T == 8, false, local_grid);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

// The template loop of this call refines level 0 on sparse bit strips: the plan of a match entry point says so and the
// record calls nothing of the level current (a reader since -- ensure_local_forms, ensure_full_lm -- would have rebuilt a form
// from the orientation map, and the loop reads that).
bool sparse_refine(const sbm_ctx* c)
{
    return c->L == 2 && c->rec.levels_valid == c->L && refine_reads(c->rec.forms[0]) == LM_NONE &&
           plan_build(plan_inputs(c), all_rows_ok(c), true).form[0] == LM_BIT_STRIPS_SPARSE;
}

// Between the coarse pass and the refinement of a sparse call: flag the tiles of level 0 that the candidates' patches lie in,
// then build the bit strips of the flagged tiles from the orientation map (the bit-strip share of k_build_lm_rows; a
// workgroup whose flag is 0 returns at once).  The unflagged tiles keep whatever an earlier call left: nothing reads them.
// The grid of the sparse gradient launch of a call of `frames` frames and how many waves per frame run it from the lists of
// working items: SBM_SPARSE_SLOTS or the default, at most the items of a frame.  slots 0: no lists, a wave per item.
// hs, n_full, n_rblocks: the launch's own grid, the FIXED grid, which a frame without a list walks, the packed waves run and the
// waves launched follow.  list_hs, list_n_rblocks: the LIST grid, the one k_mark_refine_tiles tests and lists a frame's items on.
struct SparseListPlan {
    int slots = 0, hs = 0, n_full = 0, n_rblocks = 0, list_hs = 0, list_n_rblocks = 0;
};
constexpr int SPARSE_SLOTS_DEFAULT = INT_MAX; // the items per frame (profiles/sparse_list.txt, section 5)
SparseListPlan sparse_list_plan(const sbm_ctx* c, const FrameSource& src)
{
    SparseListPlan p;
    if (!tuning().sparse_list || !c->d_items.p || !c->d_rects.p || !c->d_src0.p) return p;
    const int rows = c->rows[0], cols = c->cols[0];
    const int hs = quantize_stream_rows(c, rows, cols, src, MaskSource{}, false);
    if (!hs) return p;
    const int n_strips = (cols + QS_USEFUL - 1) / QS_USEFUL;
    const int n_full = qs_pack_lanes(rows, cols, src, MaskSource{}) ? n_strips - 1 : n_strips, n_rblocks = (rows + hs - 1) / hs;
    const int64_t per_frame = (int64_t)n_full * n_rblocks;
    if (per_frame < 1 || per_frame > c->items_cap) return p;
    p.hs = hs, p.n_full = n_full, p.n_rblocks = n_rblocks;
    p.slots = (int)std::min<int64_t>(per_frame, tuning().sparse_slots > 0 ? tuning().sparse_slots : SPARSE_SLOTS_DEFAULT);
    // The list grid.  Only a frame of few candidates has a list (at most 256, one workgroup of the mark launch), and its working
    // items follow the candidates' need rectangles: a few objects, each about a strip wide.  The estimate of the waves that work
    // in a launch of listed frames is therefore ONE strip per frame and row block, frames x ceil(rows / h) -- what works if
    // objects cover every row; fewer work where they do not, and the rule then errs towards longer items.  With that for the
    // waves, the rule of the whole-level launches (qs_rows_throughput; several batches in flight only), never longer items than
    // the fixed grid's.  The finer grid must fit the lists' room as well.
    // A context whose rows per item the caller has set (sbm_set_quantize_mode) has that one grid, unless the list grid is set too.
    const int set = c->sparse_list_rows >= 0 ? c->sparse_list_rows : tuning().sparse_list_hs;
    int list_hs = hs;
    if (set > 0) list_hs = (set + 1) & ~1;
    else if (set < 0 && !c->quantize_hs && c->pipeline_depth >= 2) list_hs = std::min(hs, qs_rows_throughput(src.frames, rows, c->n_simd));
    if (list_hs < 2 || (int64_t)n_full * ((rows + list_hs - 1) / list_hs) > c->items_cap) list_hs = hs;
    p.list_hs = list_hs, p.list_n_rblocks = (rows + list_hs - 1) / list_hs;
    return p;
}

int enqueue_sparse_strips(sbm_ctx* c, hipStream_t s, int frames)
{
    const int T = c->cfg.T[0], W = c->cols[0] / T, H = c->rows[0] / T, n_tiles = refine_tile_count(W, H), n_bands = refine_band_count(c->rows[0]);
    // the record of need rectangles only where this call's gradient launch reads it (the flags alone serve the strip builder)
    int32_t* const rects = !c->rec.map0_whole && tuning().sparse_rects ? c->d_rects.as<int32_t>() : nullptr;
    // ... and the lists of working items where that launch runs from them
    const SparseListPlan lp = rects ? sparse_list_plan(c, c->sparse_src) : SparseListPlan{};
    MarkList ml;
    memset(&ml, 0, sizeof ml);
    if (lp.slots > 0) {
        ml.items = c->d_items.as<int32_t>();
        ml.stride = refine_list_stride(c->items_cap);
        ml.capacity = (int32_t)c->items_cap;
        ml.n_full = lp.n_full, ml.n_rblocks = lp.list_n_rblocks, ml.hs = lp.list_hs, ml.useful = QS_USEFUL; // (the list grid)
    }
    SBM_LAUNCH(c, "k_mark_refine_tiles", k_mark_refine_tiles, dim3(4, frames), dim3(256), 0, s, c->d_cands.as<Cand>(), c->d_counters.as<int32_t>(),
               (int)c->cand_cap, c->rows[0], c->cols[0], T, W, H, c->d_fext.as<uint32_t>(), c->L, 0, c->d_tiles.as<uint8_t>(), n_tiles, rects, n_bands, ml);
    HIP_TRY(hipGetLastError());
    if (!c->rec.map0_whole) {
        // the call ran the source pass only (BuildPlan::sparse_gradient): level 0's gradient stage now, from the retained
        // source, in the work items whose output the flagged tiles' builders load.  The map stays in pieces (map0_whole).
        QSForm form{QS_SPARSE, nullptr, 0, c->d_tiles.as<uint8_t>(), n_tiles, T, W, H};
        form.need_rects = rects;
        form.n_bands = n_bands;
        if (lp.slots > 0) {
            form.item_list = ml.items;
            form.list_stride = ml.stride;
            form.list_cap = ml.capacity;
            form.slots = lp.slots, form.fixed_hs = lp.hs, form.list_n_full = lp.n_full, form.list_hs = lp.list_hs;
        }
        if (c->profiling && c->d_sparse_items.p) { // (no capture while profiling: graph_wanted)
            HIP_TRY(hipMemsetAsync(c->d_sparse_items.p, 0, sizeof(int32_t), s));
            form.item_count = c->d_sparse_items.as<int32_t>();
        }
        QuantizeLaunch q;
        q.src = c->sparse_src; // the caller's frames, or the retained copy (sparse_gradient_frames)
        q.rows = c->rows[0], q.cols = c->cols[0];
        q.weak = c->cfg.weak_threshold;
        q.out = c->d_quant[0].as<uint8_t>();
        q.form = &form;
        if (int e = launch_quantize(c, s, q)) return e;
    }
    LmArgs a;
    memset(&a, 0, sizeof a);
    a.n_levels = 1;
    int blocks = 0;
    a.lv[0] = lm_level_args(c, 0, LM_BIT_STRIPS_SPARSE, frames, 0, &blocks);
    if (blocks != n_tiles) return fail(SBM_ERR_STATE, "level 0: %d strip workgroups for %d refinement tiles", blocks, n_tiles);
    a.tile_flags = c->d_tiles.as<uint8_t>();
    a.n_tiles = n_tiles;
    // the last launch but one of a sparse call: where the host's count of calls enqueued is read for the NEXT call's source pass
    a.call_words = c->d_call.as<uint32_t>();
    a.call_enqueued = c->d_enqueued;
    SBM_LAUNCH(c, "k_build_lm", k_build_lm_rows, dim3(blocks, frames), dim3(256), 0, s, a);
    HIP_TRY(hipGetLastError());
    c->rec.note_level_build(0, LM_BIT_STRIPS_SPARSE, 1, a.lv[0].split, a.lv[0].allty);
    return 0;
}

// the template loop: coarse pass, then the refinement passes -- with level 0's strips built in between where the call
// holds them sparsely
int enqueue_loop(sbm_ctx* c, hipStream_t s, sbm_match_rec* d_out, int64_t cap, int32_t* d_count, int frames, bool raised)
{
    const bool sparse = sparse_refine(c);
    if (int e = enqueue_coarse(c, s, d_out, cap, d_count, frames, sparse)) return e;
    if (sparse)
        if (int e = enqueue_sparse_strips(c, s, frames)) return e;
    return enqueue_local(c, s, d_out, cap, d_count, frames, raised, sparse);
}

// The template loop on a pyramid that the stage entry points built (response planes at every level): its T = 4 refinement
// levels as bit strips too, built once per pyramid from the resident orientation map (frame 0) -- what ensure_coarse_planes is
// for the coarsest level's bit planes.  Outside any capture.
int ensure_local_forms(sbm_ctx* c, hipStream_t s)
{
    const PlanInputs pin = plan_inputs(c);
    if (int e = ensure_level0_map(c, s)) return e; // every rebuild below reads the orientation maps
    for (int l = 0; l < c->L - 1; ++l) {
        LevelForms& f = c->rec.forms[l];
        if (refine_reads(f) == LM_NONE) {
            // nothing current: a match call built the level's strips sparsely.  Whole strips from the orientation map, or the
            // response planes where strips are not wanted (any more)
            if (local_bits_wanted(pin, l) && lm_rows_ok(c->d_quant[l].as<uint8_t>(), c->cols[l], c->cfg.T[l])) {
                if (int e = c->d_lbits[l].ensure((size_t)lbits_frame_bytes(c, l), true)) return e;
                if (int e = launch_lm_level(c, s, l, LM_BIT_STRIPS)) return e;
                f.bit_strips = true;
            } else {
                if (int e = launch_build_lm(c, s, l)) return e;
                f.planes8 = true;
            }
            continue;
        }
        if (f.bit_strips) {
            // strips are current.  Asked for the byte form since, and the response planes are there: read those
            if (!local_bits_wanted(pin, l) && f.planes8) f.bit_strips = false;
            continue;
        }
        if (!local_bits_wanted(pin, l) || !f.planes8 || f.spread) continue; // only beside stage-built response planes
        if (!lm_rows_ok(c->d_quant[l].as<uint8_t>(), c->cols[l], c->cfg.T[l])) continue;
        if (int e = c->d_lbits[l].ensure((size_t)lbits_frame_bytes(c, l), true)) return e;
        if (int e = launch_lm_level(c, s, l, LM_BIT_STRIPS)) return e;
        f.bit_strips = true;
    }
    return 0;
}

// matchClass over the active templates; results into d_out/d_count (device)
int enqueue_templates(sbm_ctx* c, hipStream_t s, float threshold, sbm_match_rec* d_out, int64_t cap, int32_t* d_count)
{
    if (c->rec.levels_valid < c->L) return fail(SBM_ERR_STATE, "pyramid not built (%d of %d levels)", c->rec.levels_valid, c->L);
    if (int e = prepare_templates(c, threshold, cap)) return e;
    if (int e = ensure_local_forms(c, s)) return e;
    return enqueue_loop(c, s, d_out, cap, d_count, 1, /* raised: no gradient launches around a template-loop-only call */ true);
}

// ---- hipGraph replay of an entry point's launches -----------------------------------------------------------------
// kind: 0 single frame, > 0 frames of a batch, -1 the template loop alone
bool graph_wanted(const sbm_ctx* c, int kind)
{
    if (c->profiling) return false; // per-kernel timestamps need the launches themselves
    if (c->graph_pref == 1) return true;
    if (c->graph_pref == 0) return false;
    // auto.  Why at all: about one process in eight on this pool runs launches that alternate over several streams in a
    // slow mode (0.5 - 1.8 ms per step instead of 0.11, kernels unchanged; DESIGN.md section 9) that replay -- one host
    // call per step -- does not have; with several batches in flight the two otherwise measure the same.  A single frame
    // at a time is faster as plain launches.
    return kind != 0 && c->pipeline_depth >= 2 && !c->auto_graph_off;
}

constexpr size_t GRAPH_CACHE = 16;

// Replay the graph captured for this argument tuple on stream s, capturing it first if need be (capture(&graph) records
// the launches on the context's own stream).  *launched = false: nothing was enqueued, the caller launches on the stream
// itself -- auto mode, a tuple seen for the first time (callers whose buffers never repeat must not pay a capture per
// call) or a caller whose tuples keep changing.
template <class Capture>
int graph_replay(sbm_ctx* c, const GraphKey& key, hipStream_t s, bool* launched, Capture capture)
{
    *launched = false;
    sbm_ctx::GraphEntry* hit = nullptr;
    for (auto& g : c->graphs)
        if (g.key == key) hit = &g;
    if (!hit) {
        if (c->graph_pref < 0) {
            bool seen = false;
            for (auto& k : c->graph_seen) seen = seen || k == key;
            if (!seen) {
                if (c->graph_seen.size() >= 64) c->graph_seen.erase(c->graph_seen.begin());
                c->graph_seen.push_back(key);
                return 0;
            }
            if (++c->graph_captures_since_hit > (int)(2 * GRAPH_CACHE)) { // recurring, but more tuples than the cache holds
                c->auto_graph_off = true;
                return 0;
            }
        }
        if (c->graphs.size() >= GRAPH_CACHE) { // evict the least recently used capture
            size_t lru = 0;
            for (size_t i = 1; i < c->graphs.size(); ++i)
                if (c->graphs[i].last_use < c->graphs[lru].last_use) lru = i;
            HIP_TRY(hipDeviceSynchronize());
            (void)hipGraphExecDestroy(c->graphs[lru].exec);
            (void)hipGraphDestroy(c->graphs[lru].graph);
            c->graphs.erase(c->graphs.begin() + lru);
        }
        sbm_ctx::GraphEntry ge;
        ge.key = key;
        if (int e = capture(&ge.graph)) return e;
        hipError_t he = hipGraphInstantiate(&ge.exec, ge.graph, nullptr, nullptr, 0);
        if (he != hipSuccess) {
            (void)hipGraphDestroy(ge.graph);
            return fail(SBM_ERR_HIP, "hipGraphInstantiate failed: %s", hipGetErrorString(he));
        }
        ge.rec = c->rec; // (the capture wrote it as it enqueued)
        c->graphs.push_back(ge);
        hit = &c->graphs.back();
    } else {
        c->graph_captures_since_hit = 0;
    }
    hit->last_use = ++c->graph_clock;
    HIP_TRY(hipGraphLaunch(hit->exec, s));
    c->rec.replayed(hit->rec, key.kind);
    *launched = true;
    return 0;
}

// Ends the capture on stream m that recorded an entry point's launches with result rc: the graph, or rc's / the capture's error
int end_capture(hipStream_t m, int rc, hipGraph_t* graph)
{
    hipGraph_t g = nullptr;
    hipError_t e = hipStreamEndCapture(m, &g);
    if (rc) {
        if (g) (void)hipGraphDestroy(g);
        return rc;
    }
    if (e != hipSuccess || !g) return fail(SBM_ERR_HIP, "hipStreamEndCapture failed: %s", hipGetErrorString(e));
    *graph = g;
    return 0;
}

// A match call is counted on the device by one thread of one of its launches, behind its source pass (CALL_EXECUTED,
// sbm_lm_kernels.h): by the clearing block of the one-launch builder where the call has one, else by a launch of its own here.
// The host counts the call once its enqueue has ended (call_enqueued).
int enqueue_call_executed(sbm_ctx* c, hipStream_t s)
{
    if (c->call_counted) return 0;
    hipLaunchKernelGGL(k_call_executed, dim3(1), dim3(64), 0, s, c->d_call.as<uint32_t>(), (const uint32_t*)c->d_enqueued); // (no timing of its own)
    HIP_TRY(hipGetLastError());
    c->call_counted = true;
    return 0;
}

// The enqueue of a match call on stream s has ended, as plain launches or as the replay of its graph: the source pass of every
// call before it that has not run yet may now leave the retained copy unwritten.  The release orders the store behind everything
// the host wrote for this call.
void call_enqueued(sbm_ctx* c, hipStream_t s)
{
    c->call_recorded = c->ev_call && hipEventRecord(c->ev_call, s) == hipSuccess;
    if (!c->call_recorded) (void)hipGetLastError();
    if (c->h_enqueued) __atomic_store_n(c->h_enqueued, *c->h_enqueued + 1, __ATOMIC_RELEASE); // (the host alone writes the word)
}

// every launch of a match call, in order
int enqueue_match(sbm_ctx* c, hipStream_t s, const MatchCall& m, const Bands* bands = nullptr, bool level0_gradient_done = false)
{
    if (int e = enqueue_pyramid(c, s, m.src, m.mask, m.counts, bands, level0_gradient_done)) return e;
    if (int e = enqueue_call_executed(c, s)) return e;
    return enqueue_loop(c, s, m.out, m.cap, m.counts, m.src.frames, false);
}

// The whole match() of one frame as a DAG, recorded by stream capture on the context's two private streams:
//   main: quantize(0) -> quantize(1) -> ... -> quantize(L-1) -> build_lm(L-1) -> coarse -> [join] -> local(L-2..0)
//   side:          \-> build_lm(0)      \-> build_lm(1) ...                                  /
// The linear memories of the finer levels are only needed by the refinement passes, so their
// construction overlaps the coarse-level chain.
int enqueue_match_forked(sbm_ctx* c, const MatchCall& m)
{
    const int L = c->L;
    hipStream_t st = c->stream, sd = c->side;
    PyramidCursor cur{m.src, m.mask}; // one frame
    c->rec.begin_build(1);
    bool forked = false;
    for (int l = 0; l < L; ++l) {
        if (int e = enqueue_gradient_level(c, st, l, true, cur, 0, c->rows[l])) return e;
        const bool fork = l < L - 1 && tuning().graph_fork;
        if (fork && (hipEventRecord(c->ev_fork[l], st) != hipSuccess || hipStreamWaitEvent(sd, c->ev_fork[l], 0) != hipSuccess))
            return fail(SBM_ERR_HIP, "graph fork failed");
        forked = forked || fork;
        if (int e = launch_build_lm(c, fork ? sd : st, l)) return e;
    }
    record_build(c->rec.forms, L, plan_build(plan_inputs(c), false, true)); // the generic builder: the 8-plane form at every level
    c->rec.levels_valid = L;
    c->rec.map0_whole = true;
    c->call_counted = false;
    if (int e = enqueue_call_executed(c, st)) return e;
    if (int e = enqueue_coarse(c, st, m.out, m.cap, m.counts)) return e;
    if (forked && (hipEventRecord(c->ev_join, sd) != hipSuccess || hipStreamWaitEvent(st, c->ev_join, 0) != hipSuccess))
        return fail(SBM_ERR_HIP, "graph join failed");
    return enqueue_local(c, st, m.out, m.cap, m.counts);
}

// kind: 0 single frame, > 0 frames of a batch, -1 the template loop alone (graph_wanted).  The key of the call's captured graph:
GraphKey graph_key(const sbm_ctx* c, const MatchCall& m, int kind)
{
    GraphKey key;
    key.src = m.src;
    key.mask = m.mask;
    key.rows = m.rows, key.cols = m.cols;
    memcpy(&key.thr_bits, &m.thr, 4);
    key.out = m.out, key.cap = m.cap, key.count = m.counts;
    key.mirror_out = c->mirror_out, key.mirror_count = c->mirror_count;
    key.kind = kind;
    // (the template loop has no frames: what its launches depend on instead is the form every level is held in)
    if (kind < 0) key.forms_signature = forms_signature(c->rec.forms, c->L);
    // (a batch call whose plan makes level 0's map sparsely records other launches than a whole one at the same geometry)
    key.sparse_grad = kind > 0 && plans_sparse_gradient(c, m.src, m.mask, nullptr, false);
    key.sparse_rects = key.sparse_grad && tuning().sparse_rects && c->d_rects.p != nullptr;
    const SparseListPlan lp = key.sparse_rects ? sparse_list_plan(c, sparse_gradient_frames(c, m.src)) : SparseListPlan{};
    key.sparse_slots = lp.slots, key.sparse_list_hs = lp.slots > 0 ? lp.list_hs : 0;
    return key;
}

// The launches of a match call on stream s: a replay of the graph captured for its argument tuple where one is wanted --
// the single frame as the forked DAG, a batch (BASELINE config 5: "hipGraph-captured match loop") and the template loop as
// the plain launches recorded once on the context's stream -- else the plain launches themselves.  Every state change of
// the call has happened (begin_match; here, what only the template loop still lacks): it may synchronise, a capture cannot.
int match_or_replay(sbm_ctx* c, hipStream_t s, const MatchCall& m, int kind)
{
    if (kind != 1 && graph_wanted(c, kind)) {
        if (kind < 0) {
            if (c->rec.levels_valid < c->L) return fail(SBM_ERR_STATE, "pyramid not built (%d of %d levels)", c->rec.levels_valid, c->L);
            if (int e = prepare_templates(c, m.thr, m.cap)) return e;
            // the forms rebuilt here read the orientation maps that the caller's stream may still be writing (a match call
            // enqueued just before): launched on s, as enqueue_templates does, they are ordered after it without a host wait.
            // (prepare_templates has synchronised the context's stream whenever it enqueued anything.)
            if (int e = ensure_coarse_planes(c, s)) return e;
            if (int e = ensure_local_forms(c, s)) return e;
        }
        bool launched = false;
        const GraphKey key = graph_key(c, m, kind);
        if (int e = graph_replay(c, key, s, &launched, [&](hipGraph_t* g) {
                hipStream_t st = c->stream;
                HIP_TRY(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
                const int rc = kind == 0  ? enqueue_match_forked(c, m)
                               : kind < 0 ? enqueue_loop(c, st, m.out, m.cap, m.counts, 1, true)
                                          : enqueue_match(c, st, m);
                return end_capture(st, rc, g);
            }))
            return e;
        if (launched) {
            // (graph_replay has restored the record the capture left; the graph holds the launch that counts the call on the device)
            if (kind >= 0) call_enqueued(c, s);
            return 0;
        }
    }
    if (kind < 0) return enqueue_templates(c, s, m.thr, m.out, m.cap, m.counts);
    if (int e = enqueue_match(c, s, m)) return e;
    call_enqueued(c, s);
    return 0;
}

int fetch_results(sbm_ctx* c, hipStream_t s, sbm_match_rec* out_host, int64_t cap, int64_t* n_out)
{
    int32_t cnt[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(cnt, c->d_outcount.p, sizeof cnt, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (n_out) *n_out = cnt[0];
    if (cnt[1]) return fail(SBM_ERR_CAPACITY, "coarse candidate list overflowed (max_candidates=%lld)", (long long)c->cand_cap);
    if (cnt[0] > cap || cnt[0] > c->cand_cap)
        return fail(SBM_ERR_CAPACITY, "%d matches exceed the output capacity %lld", cnt[0], (long long)std::min<int64_t>(cap, c->cand_cap));
    if (cnt[0] > 0) {
        HIP_TRY(hipMemcpyAsync(out_host, c->d_out.p, (size_t)cnt[0] * sizeof(sbm_match_rec), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    return 0;
}

void collect_timings(sbm_ctx* c)
{
    c->timing_ms.resize(c->timings.size());
    for (size_t i = 0; i < c->timings.size(); ++i) {
        float ms = 0.f;
        (void)hipEventSynchronize(c->timings[i].b);
        (void)hipEventElapsedTime(&ms, c->timings[i].a, c->timings[i].b);
        c->timing_ms[i] = ms;
    }
}

bool feature_in_bounds(const sbm_feature& f) { return f.x >= 0 && f.y >= 0 && f.x <= 65535 && f.y <= 65535 && f.label >= 0 && f.label < 8; }

// The step both template uploads end with, after the device-wide wait: the new set becomes the context's.  sbm_upload_templates
// has written the live device tables in place (staged false); sbm_upload_templates_device has built them in c->staged, which
// changes places with the live set here.  fxy_valid false: h_fxy is fetched from d_fxy on first need.  Then what follows from
// new templates: thresholds, feature offsets and the NMS label table are stale, captured graphs hold the old tables and grid
// sizes, every class is selected.
struct TemplateCommit {
    int32_t n_templates = 0;
    int64_t n_features = 0;
    std::vector<DevTL> tls;
    std::vector<uint32_t> fxy;
    std::vector<int32_t> cls, tid;
    bool fxy_valid = true, staged = false;
};
int commit_templates(sbm_ctx* c, TemplateCommit& k)
{
    if (k.staged) {
        sbm_ctx::TemplateTables& st = c->staged;
        c->d_tls.swap(st.tls), c->d_fxy.swap(st.fxy), c->d_flabel.swap(st.flabel), c->d_flevel.swap(st.flevel);
        c->d_fxy_s.swap(st.fxy_s), c->d_flabel_s.swap(st.flabel_s), c->d_fcls.swap(st.fcls), c->d_fext.swap(st.fext);
        c->d_class.swap(st.cls), c->d_tid.swap(st.tid);
    }
    c->n_templates = k.n_templates;
    c->n_features = k.n_features;
    c->h_tls.swap(k.tls);
    c->h_fxy.swap(k.fxy);
    c->h_fxy_valid = k.fxy_valid;
    c->h_class.swap(k.cls);
    c->h_tid.swap(k.tid);
    c->have_thr = false;
    c->foff_dirty = true;
    ++c->templates_gen;
    c->drop_graphs();
    return sbm_select_classes(c, nullptr, 0);
}

} // namespace

