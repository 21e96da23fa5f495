// sbm_verify_kernels.h — the verify stage on the device (sbm_verify_batch_device*): the false-positive filter the
// reference's production driver runs on the matches NMS kept (HCORR, test_jabil.cpp:152-207): cut Rect(m.x, m.y,
// templ[0].width, templ[0].height) out of the frame, gray it, min-max normalise it to 0..255 and correlate it
// (TM_CCORR_NORMED, two images of one size: one number) with the template's normalised fiducial patch; the match counts
// where the correlation reaches min_corr.  sbm_verify_math.h holds the arithmetic.
//
// Two launches per call:
//   k_verify_rois     grid (record slots, frames), one workgroup of 1024 per ROI; slots at or past the frame's count (read
//                     here, on the device) leave at once, and a frame with more records than slots walks them by slot.
//       pass 1  the ROI's rows in quads of four pixels, consecutive lanes on consecutive quads of a row: a lane reads its
//               quad as dwords at whatever byte the row starts (12 bytes of B, G, R; 4 of a gray row or of each plane), a
//               quad that would leave the frame's row pixel by pixel.  Gray, kept in LDS where the ROI has at most VERIFY_LDS_PIXELS
//               pixels, and its minimum and maximum, reduced over the wave by shuffles and over the waves through LDS
//       table   the 256 values of rule 2 for the ROI's (lo, hi), one per thread, in LDS
//       pass 2  Sab and Saa against the stored patch, 64-bit per thread (nothing is held in 32 bits, so no ROI size
//               overflows), reduced the same way; a larger ROI reads its rows again (from L2) and grays them again
//       score   one lane applies rule 3 and writes {score, status} to the call's scratch
//   k_verify_compact  one workgroup per frame: the kept records in input order (ballot ranks, no atomic append), their
//                     scores beside them, the frame's {n_kept, flags} pair
#pragma once
#include "sbm_common.h"
#include "sbm_frame_source.h"
#include "sbm_verify_math.h"

namespace sbm {

constexpr int VERIFY_THREADS = 256;      // k_verify_compact
constexpr int VERIFY_ROI_THREADS = 1024; // k_verify_rois: sixteen waves on one ROI
constexpr int VERIFY_LDS_PIXELS = 32768; // gray bytes of a ROI held in LDS: up to 181 x 181; with the table and the
                                         // reduction words 33 KiB of a CU's 160: the waves, not LDS, bound the workgroups of a CU
constexpr int VERIFY_PATCH_PAD = 4;       // bytes behind the last patch of the store: a quad read at a patch's last pixel stays inside
constexpr int VERIFY_MAX_SLOTS = 4096;   // workgroups per frame of k_verify_rois (records past them are walked by slot)

// (class_idx, template_id) -> the label's patch: level-0 size, first byte in the patch store, sum of squares; sorted by
// (class_idx, template_id); labels without a patch are not listed
struct VerifyLabel {
    int32_t cls, tid, w, h;
    int64_t off;
    uint64_t sbb;
};

struct VerifySlot {
    float score;
    int32_t status; // VERIFY_OK, VERIFY_NO_PATCH or VERIFY_OUTSIDE
};

struct VerifyArgs {
    // frames (FrameSource): STRIDED the first frame, TABLE / PLANES the device array of addresses
    const void* base;
    int32_t kind, ch, rows, cols, stride;
    int64_t frame_stride;
    const sbm_match_rec* recs; // frame f: recs + f * cap
    const int32_t* counts;     // frame f: {count, overflow} at counts + 2 * f
    int64_t cap;
    const VerifyLabel* labels;
    int32_t n_labels;
    const uint8_t* patches;
    VerifySlot* slots; // frame f: slots + f * cap
    double min_corr;
    int32_t keep_unverified;
    sbm_match_rec* out;
    float* scores;
    int64_t out_cap;
    int32_t* out_counts;
};

__device__ __forceinline__ int verify_lookup(const VerifyLabel* __restrict__ lab, int n, int cls, int tid)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const int c = lab[mid].cls, t = lab[mid].tid;
        if (c < cls || (c == cls && t < tid)) lo = mid + 1;
        else hi = mid;
    }
    return (lo < n && lab[lo].cls == cls && lab[lo].tid == tid) ? lo : -1;
}

// the three plane (or one frame) addresses of frame f
struct VerifyFrame {
    const uint8_t* p0;
    const uint8_t* p1;
    const uint8_t* p2;
};

__device__ __forceinline__ VerifyFrame verify_frame(const VerifyArgs& A, int f)
{
    VerifyFrame v;
    if (A.kind == FRAMES_PLANES) {
        const uint8_t* const* t = (const uint8_t* const*)A.base + 3 * (size_t)f;
        v.p0 = t[0], v.p1 = t[1], v.p2 = t[2];
    } else {
        v.p0 = A.kind == FRAMES_TABLE ? ((const uint8_t* const*)A.base)[f] : (const uint8_t*)A.base + (int64_t)f * A.frame_stride;
        v.p1 = v.p2 = v.p0;
    }
    return v;
}

// gray of pixel (row, col) of the frame (rule 1)
__device__ __forceinline__ int verify_pixel(const VerifyArgs& A, const VerifyFrame& F, int row, int col)
{
    const int64_t r = (int64_t)row * A.stride;
    if (A.kind == FRAMES_PLANES) return verify_gray(F.p0[r + col], F.p1[r + col], F.p2[r + col]);
    if (A.ch == 1) return F.p0[r + col];
    const uint8_t* p = F.p0 + r + 3 * (int64_t)col;
    return verify_gray(p[0], p[1], p[2]);
}

__device__ __forceinline__ uint64_t verify_wave_sum(uint64_t v)
{
    uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const uint32_t ol = (uint32_t)__shfl_xor((int)lo, d, 64), oh = (uint32_t)__shfl_xor((int)hi, d, 64);
        const uint64_t s = (((uint64_t)hi << 32) | lo) + (((uint64_t)oh << 32) | ol);
        lo = (uint32_t)s, hi = (uint32_t)(s >> 32);
    }
    return ((uint64_t)hi << 32) | lo;
}

typedef uint32_t __attribute__((aligned(1))) verify_u32_unaligned;
__device__ __forceinline__ uint32_t verify_load4(const uint8_t* p) { return *(const verify_u32_unaligned*)p; }

// gray of the four pixels (row, col .. col + 3) of the frame, one per byte, the first lowest: 12 bytes of an interleaved row as
// three dwords at any byte address, one dword of a gray row or of each plane.  All four pixels lie inside the ROI.
__device__ __forceinline__ uint32_t verify_pixels4(const VerifyArgs& A, const VerifyFrame& F, int row, int col)
{
    const int64_t r = (int64_t)row * A.stride;
    if (A.kind == FRAMES_PLANES) {
        const uint32_t b = verify_load4(F.p0 + r + col), g = verify_load4(F.p1 + r + col), c = verify_load4(F.p2 + r + col);
        uint32_t v = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) v |= (uint32_t)verify_gray((b >> (8 * k)) & 255, (g >> (8 * k)) & 255, (c >> (8 * k)) & 255) << (8 * k);
        return v;
    }
    if (A.ch == 1) return verify_load4(F.p0 + r + col);
    const uint8_t* p = F.p0 + r + 3 * (int64_t)col;
    const uint32_t d0 = verify_load4(p), d1 = verify_load4(p + 4), d2 = verify_load4(p + 8); // B0 G0 R0 B1 | G1 R1 B2 G2 | R2 B3 G3 R3
    return (uint32_t)verify_gray(d0 & 255, (d0 >> 8) & 255, (d0 >> 16) & 255) |
           ((uint32_t)verify_gray(d0 >> 24, d1 & 255, (d1 >> 8) & 255) << 8) |
           ((uint32_t)verify_gray((d1 >> 16) & 255, d1 >> 24, d2 & 255) << 16) |
           ((uint32_t)verify_gray((d2 >> 8) & 255, (d2 >> 16) & 255, d2 >> 24) << 24);
}

// gray of up to four pixels from (row, col) on, n of them inside the ROI's row.  Where the frame's row holds four pixels from col
// on, the quad is read whole (pixels past the ROI are the frame's own, read and not counted); only at the frame's right edge are
// the n pixels read one by one, the last one again in place of the others, so that no load waits for another.
__device__ __forceinline__ uint32_t verify_quad(const VerifyArgs& A, const VerifyFrame& F, int row, int col, int n)
{
    if (col + 4 <= A.cols) return verify_pixels4(A, F, row, col);
    uint32_t v = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) v |= (uint32_t)verify_pixel(A, F, row, col + (k < n ? k : n - 1)) << (8 * k);
    return v;
}

__global__ void __launch_bounds__(VERIFY_ROI_THREADS) k_verify_rois(VerifyArgs A)
{
    constexpr int NW = VERIFY_ROI_THREADS / 64;
    __shared__ __attribute__((aligned(4))) uint8_t s_gray[VERIFY_LDS_PIXELS];
    __shared__ uint8_t s_tab[256];
    __shared__ int s_lo[NW], s_hi[NW];
    __shared__ uint64_t s_ab[NW], s_aa[NW];
    const int f = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t cnt = A.counts[2 * (size_t)f];
    const int n = (int)(cnt < 0 ? 0 : (cnt > A.cap ? A.cap : cnt));
    const VerifyFrame F = verify_frame(A, f);
    for (int slot = blockIdx.x; slot < n; slot += gridDim.x) { // (n and slot are uniform over the workgroup)
        const sbm_match_rec r = A.recs[(size_t)f * A.cap + slot];
        VerifySlot* const dst = A.slots + (size_t)f * A.cap + slot;
        const int li = verify_lookup(A.labels, A.n_labels, r.class_idx, r.template_id);
        if (li < 0) {
            if (tid == 0) *dst = VerifySlot{-1.f, VERIFY_NO_PATCH};
            continue;
        }
        const VerifyLabel L = A.labels[li];
        if (!verify_roi_inside(r.x, r.y, L.w, L.h, A.rows, A.cols)) {
            if (tid == 0) *dst = VerifySlot{-1.f, VERIFY_OUTSIDE};
            continue;
        }
        // (inside a frame whose rows * cols the host holds below 2^31: every index below is an int)
        const int w = L.w, npix = L.w * L.h, qpr = (w + 3) >> 2, nquads = qpr * L.h;
        const bool in_lds = npix <= VERIFY_LDS_PIXELS;
        // pass 1: the rows in quads of four pixels, consecutive lanes on consecutive quads of a row
        int lo = 255, hi = 0;
        for (int q = tid; q < nquads; q += VERIFY_ROI_THREADS) {
            const int y = q / qpr, x = (q - y * qpr) << 2, m = w - x < 4 ? w - x : 4;
            const uint32_t g4 = verify_quad(A, F, r.y + y, r.x + x, m);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < m) {
                    const int g = (int)((g4 >> (8 * k)) & 255);
                    if (in_lds) s_gray[y * w + x + k] = (uint8_t)g;
                    lo = g < lo ? g : lo;
                    hi = g > hi ? g : hi;
                }
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            const int ol = __shfl_xor(lo, d, 64), oh = __shfl_xor(hi, d, 64);
            lo = ol < lo ? ol : lo;
            hi = oh > hi ? oh : hi;
        }
        if (lane == 0) s_lo[wave] = lo, s_hi[wave] = hi;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < NW; ++k) {
            lo = s_lo[k] < lo ? s_lo[k] : lo;
            hi = s_hi[k] > hi ? s_hi[k] : hi;
        }
        // table
        if (tid < 256) s_tab[tid] = (uint8_t)verify_norm_entry(tid, lo, hi);
        __syncthreads();
        // pass 2: from LDS the ROI is dense, as the patch is: four pixels of both per step, whatever the rows' width; a larger
        // ROI reads its rows again
        const uint8_t* __restrict__ patch = A.patches + L.off;
        uint64_t ab = 0, aa = 0;
        if (in_lds) {
            for (int i = 4 * tid; i < npix; i += 4 * VERIFY_ROI_THREADS) {
                const int m = npix - i < 4 ? npix - i : 4;
                const uint32_t g4 = *(const uint32_t*)(s_gray + i); // (the array's tail past npix is read, not used)
                const uint32_t p4 = verify_load4(patch + i); // (the store ends in VERIFY_PATCH_PAD bytes of its own)
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (k < m) {
                        const uint32_t nv = s_tab[(g4 >> (8 * k)) & 255];
                        ab += nv * ((p4 >> (8 * k)) & 255);
                        aa += nv * nv;
                    }
            }
        } else {
            for (int q = tid; q < nquads; q += VERIFY_ROI_THREADS) {
                const int y = q / qpr, x = (q - y * qpr) << 2, m = w - x < 4 ? w - x : 4;
                const uint32_t g4 = verify_quad(A, F, r.y + y, r.x + x, m);
                const uint32_t p4 = verify_load4(patch + (int64_t)y * w + x);
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (k < m) {
                        const uint32_t nv = s_tab[(g4 >> (8 * k)) & 255];
                        ab += nv * ((p4 >> (8 * k)) & 255);
                        aa += nv * nv;
                    }
            }
        }
        ab = verify_wave_sum(ab);
        aa = verify_wave_sum(aa);
        if (lane == 0) s_ab[wave] = ab, s_aa[wave] = aa;
        __syncthreads();
        if (tid == 0) {
            uint64_t sab = 0, saa = 0;
#pragma unroll
            for (int k = 0; k < NW; ++k) sab += s_ab[k], saa += s_aa[k];
            *dst = VerifySlot{verify_score(sab, saa, L.sbb), VERIFY_OK};
        }
        __syncthreads(); // the next record rewrites every LDS array
    }
}

__global__ void __launch_bounds__(VERIFY_THREADS) k_verify_compact(VerifyArgs A)
{
    __shared__ int s_wave[VERIFY_THREADS / 64];
    __shared__ int s_flags;
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t cnt = A.counts[2 * (size_t)f], over = A.counts[2 * (size_t)f + 1];
    const int n = (int)(cnt < 0 ? 0 : (cnt > A.cap ? A.cap : cnt));
    if (tid == 0) s_flags = (cnt > A.cap || over != 0) ? 1 : 0;
    __syncthreads();
    const sbm_match_rec* __restrict__ recs = A.recs + (size_t)f * A.cap;
    const VerifySlot* __restrict__ slots = A.slots + (size_t)f * A.cap;
    sbm_match_rec* out = A.out + (size_t)f * A.out_cap;
    float* scores = A.scores + (size_t)f * A.out_cap;
    int m = 0, flags = 0; // kept so far (uniform)
    for (int base = 0; base < n; base += VERIFY_THREADS) {
        const int i = base + tid;
        bool keep = false;
        VerifySlot v{0.f, 0};
        if (i < n) {
            v = slots[i];
            flags |= v.status;
            keep = v.status == VERIFY_OK ? verify_keeps(v.score, A.min_corr) : A.keep_unverified != 0;
        }
        const uint64_t bal = __ballot(keep);
        if (lane == 0) s_wave[wave] = __popcll(bal);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int k = 0; k < VERIFY_THREADS / 64; ++k) {
            const int c = s_wave[k];
            before += k < wave ? c : 0;
            total += c;
        }
        const int pos = m + before + __popcll(bal & (((uint64_t)1 << lane) - 1));
        if (keep && pos < A.out_cap) {
            out[pos] = recs[i];
            scores[pos] = v.score;
        }
        m += total;
        __syncthreads(); // s_wave is reused
    }
    if (flags) atomicOr(&s_flags, flags); // (an OR: the order of arrival does not matter)
    __syncthreads();
    if (tid == 0) {
        A.out_counts[2 * (size_t)f] = m;
        A.out_counts[2 * (size_t)f + 1] = s_flags | (m > A.out_cap ? 2 : 0);
    }
}

} // namespace sbm
