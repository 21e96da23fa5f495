// sbm_nms_kernels.h — the match epilogue and NMS on the device (sbm_nms_batch_device): what every reference caller runs
// after Detector::match -- the epilogue's sort + std::unique (line2Dup.cpp:1142-1145) and cv_dnn::NMSBoxes over the
// boxes Rect(m.x, m.y, templ[0].width, templ[0].height) (nms.hpp; test.cpp:470-491, test_jabil.cpp:128-148).
//
// One workgroup of 1024 threads per frame:
//   gather    the frame's records of every part (n_parts lists, each clamped to cap) into one array
//   sort      bitonic sort of record indices by rec_cmp's order (similarity desc, template_id, class_idx, y, x; the
//             index breaks exact ties), padded to a power of two with a sentinel
//   compact   one pass of 1024 positions at a time: keep i iff it differs from i-1 in (x, y, similarity, class_idx)
//             (the reference's Match::operator== under std::unique) and similarity > score_threshold; ballot ranks
//             give the order-preserving slots; the first top_k survive; each survivor's box (level-0 size of its label)
//   walk      chunks of 64 candidates: the workgroup computes every candidate's maximum overlap with the boxes kept so
//             far and the chunk's 64 x 64 overlap matrix, then one wave resolves the chunk in order (nms_resolve_chunk,
//             one ballot per candidate) -- the order the adaptive threshold (eta < 1) needs
// A frame of up to NMS_LDS_MAX records keeps every array in LDS; a longer one (any cap) keeps them in global scratch
// (NmsArgs::scratch, NMS_SCRATCH_BYTES per frame) and runs the same code.
#pragma once
#include "sbm_common.h"
#include "sbm_nms_math.h"

namespace sbm {

constexpr int NMS_THREADS = 1024;
constexpr int NMS_LDS_MAX = 2048; // records of a frame held in LDS
constexpr int NMS_CHUNK = 64;
constexpr uint32_t NMS_SENTINEL = 0xffffffffu;

// (class_idx, template_id) -> level-0 (width, height), sorted by (class_idx, template_id)
struct NmsLabel {
    int32_t cls, tid, w, h;
};

struct NmsBox {
    int32_t x, y, w, h;
};

struct NmsArgs {
    const uint8_t* recs;   // part p, frame f: recs + p * part_stride + f * cap * 24
    const uint8_t* counts; // part p, frame f: {n_matches, overflow} at counts + p * part_stride + 8 * f
    int64_t cap, part_stride;
    int32_t n_parts;
    const NmsLabel* labels;
    int32_t n_labels;
    float score_threshold, nms_threshold, eta;
    int32_t top_k;
    sbm_match_rec* out;
    int64_t out_cap;
    int32_t* out_counts;
    uint8_t* scratch; // frames with more than NMS_LDS_MAX records; NMS_SCRATCH_BYTES(n_parts * cap) bytes per frame
    int64_t scratch_frame_bytes;
};

__host__ __device__ inline int64_t nms_pow2(int64_t n)
{
    int64_t p = 1;
    while (p < n) p <<= 1;
    return p;
}
__host__ __device__ inline int64_t nms_align16(int64_t b) { return (b + 15) & ~(int64_t)15; }
// scratch of one frame of at most n records: records, sort indices (power of two), candidate indices, candidate boxes,
// kept candidate positions
__host__ __device__ inline int64_t NMS_SCRATCH_BYTES(int64_t n)
{
    return nms_align16(n * (int64_t)sizeof(sbm_match_rec)) + nms_align16(nms_pow2(n) * 4) + nms_align16(n * 4) +
           nms_align16(n * (int64_t)sizeof(NmsBox)) + nms_align16(n * 4);
}

// rec_cmp of the host epilogue (sbm_capi_match.inc) as "a before b"; exact ties by position in the gathered list
__device__ __forceinline__ bool nms_before(const sbm_match_rec* __restrict__ r, uint32_t a, uint32_t b)
{
    if (b == NMS_SENTINEL) return a != NMS_SENTINEL;
    if (a == NMS_SENTINEL) return false;
    const sbm_match_rec x = r[a], y = r[b];
    if (x.similarity != y.similarity) return x.similarity > y.similarity;
    if (x.template_id != y.template_id) return x.template_id < y.template_id;
    if (x.class_idx != y.class_idx) return x.class_idx < y.class_idx;
    if (x.y != y.y) return x.y < y.y;
    if (x.x != y.x) return x.x < y.x;
    return a < b;
}

__device__ __forceinline__ bool nms_lookup(const NmsLabel* __restrict__ lab, int n, int cls, int tid, int* w, int* h)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const NmsLabel e = lab[mid];
        if (e.cls < cls || (e.cls == cls && e.tid < tid)) lo = mid + 1;
        else hi = mid;
    }
    if (lo < n && lab[lo].cls == cls && lab[lo].tid == tid) {
        *w = lab[lo].w;
        *h = lab[lo].h;
        return true;
    }
    *w = *h = 0;
    return false;
}

__device__ __forceinline__ float nms_overlap(const NmsBox a, const NmsBox b) { return nms_rect_overlap(a.x, a.y, a.w, a.h, b.x, b.y, b.w, b.h); }

// the per-frame work on arrays that live in LDS or in global scratch (inlined twice; address spaces resolve per copy)
__device__ __forceinline__ void nms_frame(const NmsArgs& A, int f, int n, sbm_match_rec* __restrict__ recs, uint32_t* __restrict__ idx,
                                          uint32_t* __restrict__ cidx, NmsBox* __restrict__ boxes, uint32_t* __restrict__ kept,
                                          float* __restrict__ ov, int* s_wave, int* s_misc, float* s_red)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // gather
    {
        int off = 0;
        for (int p = 0; p < A.n_parts; ++p) {
            const uint8_t* base = A.recs + (size_t)p * A.part_stride + (size_t)f * A.cap * sizeof(sbm_match_rec);
            const int32_t cnt = *(const int32_t*)(A.counts + (size_t)p * A.part_stride + 8 * (size_t)f);
            const int np = (int)(cnt < 0 ? 0 : (cnt > A.cap ? A.cap : cnt));
            for (int j = tid; j < np; j += NMS_THREADS) recs[off + j] = ((const sbm_match_rec*)base)[j];
            off += np;
        }
    }
    const int P = (int)nms_pow2(n);
    for (int i = tid; i < P; i += NMS_THREADS) idx[i] = i < n ? (uint32_t)i : NMS_SENTINEL;
    __syncthreads();
    // bitonic sort of the indices
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (P >> 1); t += NMS_THREADS) {
                const int i = 2 * j * (t / j) + (t % j), ixj = i + j;
                const uint32_t a = idx[i], b = idx[ixj];
                const bool up = (i & k) == 0;
                if (up ? nms_before(recs, b, a) : nms_before(recs, a, b)) {
                    idx[i] = b;
                    idx[ixj] = a;
                }
            }
            __syncthreads();
        }
    // compact: adjacent unique + score filter, order kept; first top_k; boxes
    const int limit = A.top_k > 0 ? A.top_k : 0x7fffffff;
    int m = 0; // candidates so far (uniform)
    for (int base = 0; base < n; base += NMS_THREADS) {
        const int i = base + tid;
        bool keep = false;
        uint32_t ri = 0;
        if (i < n) {
            ri = idx[i];
            const sbm_match_rec r = recs[ri];
            keep = r.similarity > A.score_threshold;
            if (keep && i > 0) {
                const sbm_match_rec q = recs[idx[i - 1]];
                keep = !(r.x == q.x && r.y == q.y && r.similarity == q.similarity && r.class_idx == q.class_idx);
            }
        }
        const uint64_t bal = __ballot(keep);
        if (lane == 0) s_wave[wave] = __popcll(bal);
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < NMS_THREADS / 64; ++w) {
            const int c = s_wave[w];
            before += w < wave ? c : 0;
            total += c;
        }
        const int pos = m + before + __popcll(bal & (((uint64_t)1 << lane) - 1));
        if (keep && pos < limit) {
            const sbm_match_rec r = recs[ri];
            int w, h;
            if (!nms_lookup(A.labels, A.n_labels, r.class_idx, r.template_id, &w, &h)) atomicOr(&s_misc[0], 4);
            cidx[pos] = ri;
            boxes[pos] = NmsBox{r.x, r.y, w, h};
        }
        m += total;
        __syncthreads(); // s_wave is reused
    }
    if (m > limit) m = limit;
    // walk
    int n_kept = 0;
    float thr = A.nms_threshold;
    sbm_match_rec* out = A.out + (size_t)f * A.out_cap;
    for (int s = 0; s < m; s += NMS_CHUNK) {
        const int cn = m - s < NMS_CHUNK ? m - s : NMS_CHUNK;
        // maximum overlap of candidate s + lane with the kept boxes: 16 slices of the kept list, one per wave
        {
            float mx = 0.f;
            if (lane < cn) {
                const NmsBox b = boxes[s + lane];
                for (int k = wave; k < n_kept; k += NMS_THREADS / 64) {
                    const float o = nms_overlap(b, boxes[kept[k]]);
                    mx = o > mx ? o : mx;
                }
            }
            s_red[wave * 64 + lane] = mx;
        }
        // the chunk's overlap matrix below the diagonal: ov[i * 64 + j] = overlap(i, j), j < i
        for (int e = tid; e < NMS_CHUNK * NMS_CHUNK; e += NMS_THREADS) {
            const int i = e >> 6, j = e & 63;
            if (j < i && i < cn) ov[e] = nms_overlap(boxes[s + i], boxes[s + j]);
        }
        __syncthreads();
        if (wave == 0) {
            float mx = 0.f;
            for (int w = 0; w < NMS_THREADS / 64; ++w) mx = s_red[w * 64 + lane] > mx ? s_red[w * 64 + lane] : mx;
            // lane j holds column j of the matrix, the diagonal being the candidate's overlap with earlier chunks
            float col[NMS_CHUNK];
#pragma unroll
            for (int i = 0; i < NMS_CHUNK; ++i) col[i] = i == lane ? (n_kept ? mx : 0.f) : ov[i * 64 + lane];
            const int nk0 = n_kept;
            const uint64_t km = nms_resolve_chunk(cn, &thr, A.eta, [&](int i, float t) -> uint64_t {
                const bool v = (i == lane && nk0 == 0) ? false : col[i] > t;
                return __ballot(v && lane <= i);
            });
            if ((km >> lane) & 1) {
                const int k = n_kept + __popcll(km & (((uint64_t)1 << lane) - 1));
                kept[k] = (uint32_t)(s + lane);
                if (k < A.out_cap) out[k] = recs[cidx[s + lane]];
            }
            if (lane == 0) {
                s_misc[1] = n_kept + __popcll(km);
                *(float*)&s_misc[2] = thr;
            }
        }
        __syncthreads();
        n_kept = s_misc[1];
        thr = *(const float*)&s_misc[2];
        __syncthreads(); // s_misc / s_red / ov are rewritten by the next chunk
    }
    if (tid == 0) {
        int flags = s_misc[0];
        if (n_kept > A.out_cap) flags |= 2;
        A.out_counts[2 * f] = n_kept;
        A.out_counts[2 * f + 1] = flags;
    }
}

__global__ void __launch_bounds__(NMS_THREADS) k_nms_frames(NmsArgs A)
{
    __shared__ sbm_match_rec s_recs[NMS_LDS_MAX];
    __shared__ uint32_t s_idx[NMS_LDS_MAX];
    __shared__ uint32_t s_cidx[NMS_LDS_MAX];
    __shared__ NmsBox s_boxes[NMS_LDS_MAX];
    __shared__ uint32_t s_kept[NMS_LDS_MAX];
    __shared__ float s_ov[NMS_CHUNK * NMS_CHUNK];
    __shared__ float s_red[NMS_THREADS];
    __shared__ int s_wave[NMS_THREADS / 64];
    __shared__ int s_misc[4];
    const int f = blockIdx.x;
    // records of the frame and the overflow flag (bit 0)
    int n = 0, flags = 0;
    for (int p = 0; p < A.n_parts; ++p) {
        const int32_t* c = (const int32_t*)(A.counts + (size_t)p * A.part_stride + 8 * (size_t)f);
        const int32_t cnt = c[0];
        if (cnt > A.cap || c[1] != 0) flags |= 1;
        n += (int)(cnt < 0 ? 0 : (cnt > A.cap ? A.cap : cnt));
    }
    if (threadIdx.x == 0) s_misc[0] = flags;
    __syncthreads();
    if (n <= NMS_LDS_MAX) {
        nms_frame(A, f, n, s_recs, s_idx, s_cidx, s_boxes, s_kept, s_ov, s_wave, s_misc, s_red);
    } else {
        uint8_t* sc = A.scratch + (size_t)f * A.scratch_frame_bytes;
        const int64_t N = (int64_t)A.n_parts * A.cap;
        sbm_match_rec* recs = (sbm_match_rec*)sc;
        uint32_t* idx = (uint32_t*)(sc + nms_align16(N * (int64_t)sizeof(sbm_match_rec)));
        uint32_t* cidx = idx + nms_align16(nms_pow2(N) * 4) / 4;
        NmsBox* boxes = (NmsBox*)(cidx + nms_align16(N * 4) / 4);
        uint32_t* kept = (uint32_t*)(boxes + nms_align16(N * (int64_t)sizeof(NmsBox)) / (int64_t)sizeof(NmsBox));
        nms_frame(A, f, n, recs, idx, cidx, boxes, kept, s_ov, s_wave, s_misc, s_red);
    }
}

} // namespace sbm
