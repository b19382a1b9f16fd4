// Batched NMS on gfx950: utils/general.py:629-711 including the torchvision.ops.nms core (:694).
//
// Per image, entirely on the device (the reference loops over images in Python with nonzero() syncs):
//   1. count   candidates per 1024-row chunk           (obj > thr, then obj*cls > thr per class / best class)
//   2. scan    chunk counts -> offsets                  (compaction order == prediction order: box-major, class-minor)
//   3. emit    key = ~bits(score), val = row*nc + cls   (8 B per candidate; boxes are re-derived from `pred` when needed)
//   4. select  three-level radix select of the exact top max_nms = 30000 (:688-689) + order-preserving compaction
//      sort    parallel rank sort of the <= 30000 survivors, stable (ties keep prediction order = the oracle's
//              stable descending sort)
//   5. greedy  512 candidates per round: test against the kept list (LDS), build the round's 512x512 suppression bit
//              matrix, resolve it serially in one wave, append survivors; stop at max_det kept (:696-697).
// What follows the sort is selectable (somi_nms_ex_f32, somi_nms_boxes_f32); stages 1-4 are shared by every mode:
//   greedy<MODE>  the same round / bit-matrix kernel with the overlap test of the reference's NMS() (general.py:925-951):
//              suppress iff !(bbox_iou(kept, cand, GIoU|DIoU|CIoU|EIoU|SIoU) <= thr), utils/metrics.py:490-579 at alpha = 1.
//   soft       Soft-NMS (general.py:834-862 with box_iou_for_nms CIoU, :868-892): one workgroup per image, one pass over
//              the live candidates and one block-wide argmax per pick, at most max_det picks.
//   merge      merge-NMS (general.py:698-704): one workgroup per kept box, fixed-order weighted mean, then the
//              `redundant` compaction.
// IoU arithmetic is written with explicit round-to-nearest intrinsics (no FMA contraction) in the oracle's operation
// order, so the kept index lists are bit-exact: area=(x2-x1)*(y2-y1) on class-offset boxes (offset 4096*cls, :692-693),
// inter=max(0,min(x2)-max(x1))*max(0,min(y2)-max(y1)), iou=inter/((area_i+area_j)-inter), suppress iff iou > thr.
#include "common.h"

namespace somi {

constexpr int NMS_CHUNK = 512;       // rows per count/emit workgroup (256 threads x 2 consecutive rows)
constexpr int MAX_NMS = 30000;       // utils/general.py:641
constexpr float MAX_WH = 4096.f;     // utils/general.py:640
constexpr int ROUND = 512;           // candidates per greedy round
constexpr int MAX_DET_CAP = 1024;
constexpr int NMS_MASK_WORDS = 16;   // class filter bit array: nc <= 1024

enum { NMS_IOU = 0, NMS_GIOU, NMS_DIOU, NMS_CIOU, NMS_EIOU, NMS_SIOU, NMS_SOFT, NMS_MODES };   // SOMI_NMS_* of somi_hip.h

struct NmsArgs {
    const float *pred;
    int B, n, nc, no;
    float conf_thres, iou_thres;
    int multi_label, agnostic, max_det;
    uint64_t classes_mask[NMS_MASK_WORDS];   // bit c of word c/64 set = keep class c
    int nchunk, cap;                 // cap = candidate capacity per image
    int *chunk_cnt;                  // [B][nchunk]
    int *chunk_off;                  // [B][nchunk]
    int *total;                      // [B]
    uint32_t *keyA, *valA, *keyB, *valB;   // [B][cap]
    float *det;                      // [B][max_det][6]
    int32_t *count;                  // [B]
    // boxes + scores form (somi_nms_boxes_f32: the reference's standalone NMS() / soft_nms()); NULL in the pipeline
    const float *boxes;              // [n][4] xyxy
    float *scores;                   // [n], decayed in place by Soft-NMS
    int64_t *keep;                   // [n] kept indices
    struct BoxO *kept_g;             // [n] kept list of the greedy kernel (the pipeline keeps its <= max_det in LDS)
    float sigma, score_thres;        // Soft-NMS
};

__device__ __forceinline__ bool class_ok(const uint64_t *mask, int c) { return (mask[c >> 6] >> (c & 63)) & 1ull; }

// number of entries row r contributes; optionally writes them (keys/vals) starting at dst
template <bool EMIT>
__device__ __forceinline__ int row_entries(const NmsArgs &a, const float *row, int r, uint32_t *keys, uint32_t *vals, int dst) {
    const float obj = row[4];
    if (!(obj > a.conf_thres)) return 0;
    int cnt = 0;
    if (a.multi_label) {
        for (int j = 0; j < a.nc; ++j) {
            const float conf = __fmul_rn(row[5 + j], obj);
            if (conf > a.conf_thres && class_ok(a.classes_mask, j)) {
                if (EMIT) {
                    keys[dst + cnt] = ~__float_as_uint(conf);
                    vals[dst + cnt] = (uint32_t)r * (uint32_t)a.nc + (uint32_t)j;
                }
                ++cnt;
            }
        }
    } else {
        float best = __fmul_rn(row[5], obj);
        int bj = 0;
        for (int j = 1; j < a.nc; ++j) {
            const float conf = __fmul_rn(row[5 + j], obj);
            if (conf > best) { best = conf; bj = j; }          // first maximum wins, like torch.max
        }
        if (best > a.conf_thres && class_ok(a.classes_mask, bj)) {
            if (EMIT) {
                keys[dst] = ~__float_as_uint(best);
                vals[dst] = (uint32_t)r * (uint32_t)a.nc + (uint32_t)bj;
            }
            cnt = 1;
        }
    }
    return cnt;
}

// block-wide exclusive scan of one int per thread (256 threads); returns the exclusive prefix, total in *tot
__device__ __forceinline__ int block_exscan_256(int v, int *tot, int *lds /* >= 4 ints */) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o);
        if (lane >= o) inc += t;
    }
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    int base = 0;
    for (int w = 0; w < wave; ++w) base += lds[w];
    *tot = lds[0] + lds[1] + lds[2] + lds[3];
    __syncthreads();
    return base + inc - v;
}

// count (EMIT=false) / emit (EMIT=true) over one chunk of NMS_CHUNK prediction rows.  The chunk's rows are staged in LDS
// with coalesced 16 B loads (a row is 4*(5+nc) bytes, so per-thread row reads straight from HBM touch every line many
// times: PMC showed 9.1 GB fetched for 0.26 GB of predictions); emitted (key, val) pairs are compacted in LDS and leave
// as contiguous stores.
constexpr int EMIT_STAGE = 4096;     // (key,val) pairs staged per chunk before falling back to direct stores
__global__ void nms_scan_kernel(const NmsArgs a);

// RPT = rows per thread (chunk = 256 * RPT rows); STAGE = false reads the rows straight from HBM (heads too wide for the LDS
// staging: nc > 110) and keeps only the emit staging in LDS.
template <bool EMIT, int RPT, bool STAGE>
__global__ __launch_bounds__(256) void nms_count_emit_kernel(const NmsArgs a) {
    extern __shared__ __attribute__((aligned(16))) float rows[];     // [256 * RPT][no] (STAGE), then the emit staging
    __shared__ int lds[4];
    constexpr int CHUNK = 256 * RPT;
    const int chunk = blockIdx.x, b = blockIdx.y;
    const int rbase = chunk * CHUNK;
    const int nrow = min(CHUNK, a.n - rbase);
    const float *src = a.pred + ((size_t)b * a.n + rbase) * a.no;
    if (STAGE) {
        const int nfl = nrow * a.no;
        if (((reinterpret_cast<uintptr_t>(src) & 15u) == 0)) {
            for (int i = threadIdx.x * 4; i + 3 < nfl; i += 1024)
                *reinterpret_cast<float4 *>(rows + i) = *reinterpret_cast<const float4 *>(src + i);
            for (int i = (nfl & ~3) + threadIdx.x; i < nfl; i += 256) rows[i] = src[i];
        } else {
            for (int i = threadIdx.x; i < nfl; i += 256) rows[i] = src[i];
        }
        __syncthreads();
    }
    const float *rsrc = STAGE ? rows : src;
    const int rl0 = threadIdx.x * RPT;
    int cnt[RPT], mine = 0;
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
        const int rl = rl0 + i;
        cnt[i] = rl < nrow ? row_entries<false>(a, rsrc + (size_t)rl * a.no, rbase + rl, nullptr, nullptr, 0) : 0;
        mine += cnt[i];
    }
    int tot;
    const int pre = block_exscan_256(mine, &tot, lds);
    if (!EMIT) {
        if (threadIdx.x == 0) a.chunk_cnt[b * a.nchunk + chunk] = tot;
        return;
    }
    const int gbase = a.chunk_off[b * a.nchunk + chunk];
    uint32_t *keys = a.keyA + (size_t)b * a.cap, *vals = a.valA + (size_t)b * a.cap;
    if (tot <= EMIT_STAGE) {
        uint32_t *skey = reinterpret_cast<uint32_t *>(rows + (STAGE ? CHUNK * a.no : 0)), *sval = skey + EMIT_STAGE;
        int dst = pre;
#pragma unroll
        for (int i = 0; i < RPT; ++i) {
            const int rl = rl0 + i;
            if (cnt[i]) row_entries<true>(a, rsrc + (size_t)rl * a.no, rbase + rl, skey, sval, dst);
            dst += cnt[i];
        }
        __syncthreads();
        for (int i = threadIdx.x; i < tot; i += 256) {
            keys[gbase + i] = skey[i];
            vals[gbase + i] = sval[i];
        }
    } else {
        int dst = gbase + pre;
#pragma unroll
        for (int i = 0; i < RPT; ++i) {
            const int rl = rl0 + i;
            if (cnt[i]) row_entries<true>(a, rsrc + (size_t)rl * a.no, rbase + rl, keys, vals, dst);
            dst += cnt[i];
        }
    }
}

// rows per count/emit workgroup for a head of nc classes: the largest of 512 / 256 whose LDS image (+ emit staging) fits
static int nms_chunk_rows(int nc) { return ((size_t)NMS_CHUNK * (nc + 5) * 4 + (size_t)EMIT_STAGE * 8 <= 150 * 1024) ? NMS_CHUNK : 256; }
static bool nms_rows_staged(int nc) { return (size_t)nms_chunk_rows(nc) * (nc + 5) * 4 + (size_t)EMIT_STAGE * 8 <= 150 * 1024; }

template <int RPT, bool STAGE>
static void launch_count_emit(const NmsArgs &a, hipStream_t s) {
    const size_t rows_lds = STAGE ? (size_t)256 * RPT * a.no * 4 : 0, emit_lds = rows_lds + (size_t)EMIT_STAGE * 8;
    if (emit_lds > 64 * 1024) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&nms_count_emit_kernel<false, RPT, STAGE>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)rows_lds);
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&nms_count_emit_kernel<true, RPT, STAGE>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)emit_lds);
    }
    hipLaunchKernelGGL((nms_count_emit_kernel<false, RPT, STAGE>), dim3(a.nchunk, a.B), dim3(256), rows_lds, s, a);
    hipLaunchKernelGGL(nms_scan_kernel, dim3(a.B), dim3(256), 0, s, a);
    hipLaunchKernelGGL((nms_count_emit_kernel<true, RPT, STAGE>), dim3(a.nchunk, a.B), dim3(256), emit_lds, s, a);
}

__global__ __launch_bounds__(256) void nms_scan_kernel(const NmsArgs a) {
    __shared__ int lds[4];
    __shared__ int carry;
    const int b = blockIdx.x;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int c0 = 0; c0 < a.nchunk; c0 += 256) {
        const int c = c0 + threadIdx.x;
        const int v = c < a.nchunk ? a.chunk_cnt[b * a.nchunk + c] : 0;
        int tot;
        const int pre = block_exscan_256(v, &tot, lds);
        if (c < a.nchunk) a.chunk_off[b * a.nchunk + c] = carry + pre;
        __syncthreads();
        if (threadIdx.x == 0) carry += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) a.total[b] = carry;
}

// ------------------------------------------------------------------------------------------------ top-k select
// Only the first max_nms = 30000 entries of the (score desc, prediction order) ranking are used (general.py:688-689).
// A three-level radix select (12 + 12 + 8 key bits, histograms in LDS then merged with global atomics) finds the
// exact 32-bit threshold key T of the 30000-th entry; an order-preserving compaction then keeps every entry with
// key < T plus the first r entries with key == T.  Images with <= 30000 candidates skip all of this.
constexpr int SEL_CHUNK = 4096;      // candidates per select workgroup (256 threads x 16)

struct SelState {                    // per image, in global memory (zeroed every call)
    int hist1[4096];
    int hist2[4096];
    int hist3[256];
};

// exclusive prefix search over a histogram in global memory by one workgroup of 256 threads:
// returns the first bin whose inclusive cumulative count exceeds `need` (0-based rank), and the count before it.
__device__ __forceinline__ void find_bin(const int *hist, int nbins, int need, int *bin_out, int *before_out, int *lds) {
    // lds: >= 260 ints
    const int tid = threadIdx.x;
    const int per = nbins / 256;                   // 16 or 1
    int s = 0;
    for (int i = 0; i < per; ++i) s += hist[tid * per + i];
    int tot;
    const int pre = block_exscan_256(s, &tot, lds);
    __shared__ int res[2];
    if (need >= pre && need < pre + s) {           // exactly one thread
        int run = pre;
        for (int i = 0; i < per; ++i) {
            const int c = hist[tid * per + i];
            if (need < run + c) { res[0] = tid * per + i; res[1] = run; break; }
            run += c;
        }
    }
    __syncthreads();
    *bin_out = res[0];
    *before_out = res[1];
    __syncthreads();
}

// level 1/2/3 histogram kernels: grid (nsel_chunks, B)
template <int LEVEL>
__global__ __launch_bounds__(256) void nms_select_hist_kernel(const NmsArgs a, SelState *st) {
    __shared__ int lh[4096];
    __shared__ int lds[264];
    const int b = blockIdx.y;
    const int n = a.total[b];
    if (n <= MAX_NMS) return;
    const int i0 = blockIdx.x * SEL_CHUNK;
    if (i0 >= n) return;
    SelState &S = st[b];
    uint32_t prefix = 0;
    if (LEVEL >= 2) {
        int b1, bef1;
        find_bin(S.hist1, 4096, MAX_NMS - 1, &b1, &bef1, lds);
        prefix = (uint32_t)b1 << 20;
        if (LEVEL == 3) {
            int b2, bef2;
            find_bin(S.hist2, 4096, MAX_NMS - 1 - bef1, &b2, &bef2, lds);
            prefix |= (uint32_t)b2 << 8;
        }
    }
    constexpr int NB = LEVEL == 3 ? 256 : 4096;
    for (int i = threadIdx.x; i < NB; i += 256) lh[i] = 0;
    __syncthreads();
    const uint32_t *keys = a.keyA + (size_t)b * a.cap;
    const int i1 = min(i0 + SEL_CHUNK, n);
    for (int i = i0 + threadIdx.x; i < i1; i += 256) {
        const uint32_t k = keys[i];
        if (LEVEL == 1) atomicAdd(&lh[k >> 20], 1);
        else if (LEVEL == 2) { if ((k >> 20) == (prefix >> 20)) atomicAdd(&lh[(k >> 8) & 0xFFFu], 1); }
        else { if ((k >> 8) == (prefix >> 8)) atomicAdd(&lh[k & 0xFFu], 1); }
    }
    __syncthreads();
    int *gh = LEVEL == 1 ? S.hist1 : (LEVEL == 2 ? S.hist2 : S.hist3);
    for (int i = threadIdx.x; i < NB; i += 256)
        if (lh[i]) atomicAdd(&gh[i], lh[i]);
}

// threshold key T and number of ties r to take, recomputed by whoever needs them
__device__ __forceinline__ void select_threshold(const SelState &S, uint32_t *T, int *r, int *lds) {
    int b1, bef1, b2, bef2, b3, bef3;
    find_bin(S.hist1, 4096, MAX_NMS - 1, &b1, &bef1, lds);
    find_bin(S.hist2, 4096, MAX_NMS - 1 - bef1, &b2, &bef2, lds);
    find_bin(S.hist3, 256, MAX_NMS - 1 - bef1 - bef2, &b3, &bef3, lds);
    *T = ((uint32_t)b1 << 20) | ((uint32_t)b2 << 8) | (uint32_t)b3;
    *r = MAX_NMS - (bef1 + bef2 + bef3);           // entries with key == T to keep (>= 1)
}

// order-preserving compaction in three steps (count -> scan -> write) over SEL_CHUNK-sized chunks.
// sel_cnt[b][chunk] = {#key<T, #key==T}; after the scan kernel: exclusive prefixes.
template <bool WRITE>
__global__ __launch_bounds__(256) void nms_select_compact_kernel(const NmsArgs a, const SelState *st, int2 *sel_cnt,
                                                                 int nsel_chunk) {
    __shared__ int lds[264];
    const int b = blockIdx.y, chunk = blockIdx.x;
    const int n = a.total[b];
    if (n <= MAX_NMS) return;
    const int i0 = chunk * SEL_CHUNK + threadIdx.x * 16;       // 16 consecutive candidates per thread
    uint32_t T;
    int r;
    select_threshold(st[b], &T, &r, lds);
    const uint32_t *keys = a.keyA + (size_t)b * a.cap;
    const uint32_t *vals = a.valA + (size_t)b * a.cap;
    uint32_t k[16];
    int lt = 0, eq = 0;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int i = i0 + e;
        k[e] = i < n ? keys[i] : 0xFFFFFFFFu;
        lt += (i < n && k[e] < T) ? 1 : 0;
        eq += (i < n && k[e] == T) ? 1 : 0;
    }
    int tot_lt, tot_eq;
    const int pre_lt = block_exscan_256(lt, &tot_lt, lds);
    const int pre_eq = block_exscan_256(eq, &tot_eq, lds);
    if (!WRITE) {
        if (threadIdx.x == 0) sel_cnt[b * nsel_chunk + chunk] = make_int2(tot_lt, tot_eq);
        return;
    }
    const int2 base = sel_cnt[b * nsel_chunk + chunk];          // exclusive prefixes over chunks
    int eq_rank = base.y + pre_eq;                               // rank among ties, in prediction order
    // destination: entries keep their relative order: position = (#selected before me)
    // selected-before = lt_before + min(eq_before, r)
    int lt_rank = base.x + pre_lt;
    uint32_t *ok_ = a.keyB + (size_t)b * a.cap, *ov = a.valB + (size_t)b * a.cap;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int i = i0 + e;
        if (i >= n) break;
        const bool is_lt = k[e] < T, is_eq = k[e] == T;
        if (is_lt || (is_eq && eq_rank < r)) {
            const int pos = lt_rank + min(eq_rank, r);
            ok_[pos] = k[e];
            ov[pos] = vals[i];
        }
        lt_rank += is_lt ? 1 : 0;
        eq_rank += is_eq ? 1 : 0;
    }
}

__global__ __launch_bounds__(256) void nms_select_scan_kernel(const NmsArgs a, int2 *sel_cnt, int nsel_chunk) {
    __shared__ int lds[8];
    __shared__ int carry[2];
    const int b = blockIdx.x;
    if (a.total[b] <= MAX_NMS) return;
    if (threadIdx.x == 0) carry[0] = carry[1] = 0;
    __syncthreads();
    const int used = (a.total[b] + SEL_CHUNK - 1) / SEL_CHUNK;
    for (int c0 = 0; c0 < used; c0 += 256) {
        const int c = c0 + threadIdx.x;
        const int2 v = c < used ? sel_cnt[b * nsel_chunk + c] : make_int2(0, 0);
        int tx, ty;
        const int px = block_exscan_256(v.x, &tx, lds);
        const int py = block_exscan_256(v.y, &ty, lds);
        if (c < used) sel_cnt[b * nsel_chunk + c] = make_int2(carry[0] + px, carry[1] + py);
        __syncthreads();
        if (threadIdx.x == 0) { carry[0] += tx; carry[1] += ty; }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------ rank sort
// Stable sort of the (<= 30000) selected entries by (key, position): every entry counts the entries that precede it.
// grid (ceil(30000/256), B); the candidate keys stream through LDS in tiles of 2048.  O(n^2) compares spread over the
// whole chip (n = 30000: 9e8 compares per image), deterministic, no atomics.  Output: sorted vals -> sortV.
__global__ __launch_bounds__(256) void nms_rank_sort_kernel(const NmsArgs a, uint32_t *sortV) {
    __shared__ uint32_t tile[2048];
    const int b = blockIdx.y;
    const int tot = a.total[b];
    const bool sel = tot > MAX_NMS;
    const int n = sel ? MAX_NMS : tot;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (blockIdx.x * 256 >= n) return;
    const uint32_t *keys = (sel ? a.keyB : a.keyA) + (size_t)b * a.cap;
    const uint32_t *vals = (sel ? a.valB : a.valA) + (size_t)b * a.cap;
    const uint32_t mine = i < n ? keys[i] : 0xFFFFFFFFu;
    int rank = 0;
    for (int j0 = 0; j0 < n; j0 += 2048) {
        const int m = min(2048, n - j0);
        __syncthreads();
        for (int t = threadIdx.x; t < m; t += 256) tile[t] = keys[j0 + t];
        __syncthreads();
        // entries before me in position with key <= mine, entries after me with key < mine
        const int split = min(max(i - j0, 0), m);          // tile positions [0,split) precede me
        int cnt = 0;
        for (int t = 0; t < split; ++t) cnt += tile[t] <= mine ? 1 : 0;
        for (int t = split; t < m; ++t) cnt += tile[t] < mine ? 1 : 0;
        rank += cnt;
    }
    if (i < n) sortV[(size_t)b * MAX_NMS + rank] = vals[i];
}

// ------------------------------------------------------------------------------------------------ greedy NMS
struct BoxO { float x1, y1, x2, y2, area; };   // class-offset corners + area

__device__ __forceinline__ bool iou_gt(const BoxO &p, const BoxO &q, float thr) {
    const float xx1 = fmaxf(p.x1, q.x1), yy1 = fmaxf(p.y1, q.y1);
    const float xx2 = fminf(p.x2, q.x2), yy2 = fminf(p.y2, q.y2);
    const float iw = fmaxf(0.f, __fsub_rn(xx2, xx1)), ih = fmaxf(0.f, __fsub_rn(yy2, yy1));
    const float inter = __fmul_rn(iw, ih);
    const float iou = __fdiv_rn(inter, __fsub_rn(__fadd_rn(p.area, q.area), inter));
    return iou > thr;
}

// utils/metrics.py bbox_iou(box1 = p, box2 = q, x1y1x2y2=True, <MODE>=True) at alpha = 1, eps = 1e-7, operation for operation (:490-579):
// `h + eps`, `union + eps` and then `inter / (union + eps)`; the `** alpha` / `pow(., alpha)` steps are exact at alpha = 1.  GIoU, DIoU and
// EIoU use only + - * / min max, so with the round-to-nearest intrinsics they reproduce the CPU's bits; CIoU and SIoU go through atan /
// asin / cos / exp, which agree with the CPU's libm to a few roundings only.  Python scalars enter torch's fp32 kernels rounded to fp32.
constexpr float IOU_EPS = 1e-7f;
constexpr float CIOU_K = (float)(4.0 / (3.141592653589793 * 3.141592653589793));     // 4 / math.pi ** 2
constexpr float ONE_EPS = (float)(1.0 + 1e-7);                                       // (1 + eps)
constexpr float HALF_PI = (float)(3.141592653589793 / 2.0);
constexpr float SIN45 = (float)(1.4142135623730951 / 2.0);                           // pow(2, 0.5) / 2

__device__ __forceinline__ float sq_rn(float x) { return __fmul_rn(x, x); }

template <int MODE>
__device__ __forceinline__ float bbox_iou_ref(const BoxO &p, const BoxO &q) {
    const float iw = fmaxf(0.f, __fsub_rn(fminf(p.x2, q.x2), fmaxf(p.x1, q.x1)));
    const float ih = fmaxf(0.f, __fsub_rn(fminf(p.y2, q.y2), fmaxf(p.y1, q.y1)));
    const float inter = __fmul_rn(iw, ih);
    const float w1 = __fsub_rn(p.x2, p.x1), h1 = __fadd_rn(__fsub_rn(p.y2, p.y1), IOU_EPS);
    const float w2 = __fsub_rn(q.x2, q.x1), h2 = __fadd_rn(__fsub_rn(q.y2, q.y1), IOU_EPS);
    const float uni = __fadd_rn(__fsub_rn(__fadd_rn(__fmul_rn(w1, h1), __fmul_rn(w2, h2)), inter), IOU_EPS);
    const float iou = __fdiv_rn(inter, __fadd_rn(uni, IOU_EPS));
    const float cw = __fsub_rn(fmaxf(p.x2, q.x2), fminf(p.x1, q.x1));
    const float ch = __fsub_rn(fmaxf(p.y2, q.y2), fminf(p.y1, q.y1));
    if (MODE == NMS_GIOU) {
        const float c_area = __fadd_rn(__fmul_rn(cw, ch), IOU_EPS);
        return __fsub_rn(iou, __fadd_rn(__fdiv_rn(__fsub_rn(c_area, uni), c_area), IOU_EPS));
    }
    const float c2 = __fadd_rn(__fadd_rn(sq_rn(cw), sq_rn(ch)), IOU_EPS);
    const float dx = __fsub_rn(__fsub_rn(__fadd_rn(q.x1, q.x2), p.x1), p.x2);
    const float dy = __fsub_rn(__fsub_rn(__fadd_rn(q.y1, q.y2), p.y1), p.y2);
    const float rho2 = __fdiv_rn(__fadd_rn(sq_rn(dx), sq_rn(dy)), 4.f);
    if (MODE == NMS_DIOU) return __fsub_rn(iou, __fdiv_rn(rho2, c2));
    if (MODE == NMS_CIOU) {
        const float v = __fmul_rn(CIOU_K, sq_rn(__fsub_rn(atanf(__fdiv_rn(w2, h2)), atanf(__fdiv_rn(w1, h1)))));
        const float alpha = __fdiv_rn(v, __fadd_rn(__fsub_rn(v, iou), ONE_EPS));
        return __fsub_rn(iou, __fadd_rn(__fdiv_rn(rho2, c2), __fadd_rn(__fmul_rn(v, alpha), IOU_EPS)));
    }
    if (MODE == NMS_EIOU) {
        const float rho_w2 = sq_rn(__fsub_rn(__fsub_rn(q.x2, q.x1), __fsub_rn(p.x2, p.x1)));
        const float rho_h2 = sq_rn(__fsub_rn(__fsub_rn(q.y2, q.y1), __fsub_rn(p.y2, p.y1)));
        const float cw2 = __fadd_rn(sq_rn(cw), IOU_EPS), ch2 = __fadd_rn(sq_rn(ch), IOU_EPS);
        return __fsub_rn(iou, __fadd_rn(__fadd_rn(__fdiv_rn(rho2, c2), __fdiv_rn(rho_w2, cw2)), __fdiv_rn(rho_h2, ch2)));
    }
    // SIoU (:540-559)
    const float s_cw = __fadd_rn(__fmul_rn(dx, 0.5f), IOU_EPS), s_ch = __fadd_rn(__fmul_rn(dy, 0.5f), IOU_EPS);
    const float sigma = __fsqrt_rn(__fadd_rn(sq_rn(s_cw), sq_rn(s_ch)));
    const float sin1 = __fdiv_rn(fabsf(s_cw), sigma), sin2 = __fdiv_rn(fabsf(s_ch), sigma);
    const float sin_alpha = sin1 > SIN45 ? sin2 : sin1;
    const float angle_cost = cosf(__fsub_rn(__fmul_rn(asinf(sin_alpha), 2.f), HALF_PI));
    const float rho_x = sq_rn(__fdiv_rn(s_cw, cw)), rho_y = sq_rn(__fdiv_rn(s_ch, ch));
    const float gamma = __fsub_rn(angle_cost, 2.f);
    const float distance_cost = __fsub_rn(__fsub_rn(2.f, expf(__fmul_rn(gamma, rho_x))), expf(__fmul_rn(gamma, rho_y)));
    const float omiga_w = __fdiv_rn(fabsf(__fsub_rn(w1, w2)), fmaxf(w1, w2));
    const float omiga_h = __fdiv_rn(fabsf(__fsub_rn(h1, h2)), fmaxf(h1, h2));
    const float ew = __fsub_rn(1.f, expf(-omiga_w)), eh = __fsub_rn(1.f, expf(-omiga_h));
    const float shape_cost = __fadd_rn(sq_rn(sq_rn(ew)), sq_rn(sq_rn(eh)));
    return __fsub_rn(iou, __fadd_rn(__fmul_rn(0.5f, __fadd_rn(distance_cost, shape_cost)), IOU_EPS));
}

// does the kept box p suppress the later candidate q?  NMS_IOU is the torchvision rule (iou > thr); the penalised modes follow
// general.py:948, where a candidate survives iff metric <= thr, so a NaN suppresses
template <int MODE>
__device__ __forceinline__ bool suppresses(const BoxO &p, const BoxO &q, float thr) {
    if (MODE == NMS_IOU) return iou_gt(p, q, thr);
    return !(bbox_iou_ref<MODE>(p, q) <= thr);
}

// general.py box_iou_for_nms(box1 = p, box2 = q, CIoU=True), :868-892: h clamped at eps, one `+ eps` on the union
__device__ __forceinline__ float ciou_for_soft_nms(const float4 &p, const float4 &q) {
    const float w1 = __fsub_rn(p.z, p.x), h1 = fmaxf(__fsub_rn(p.w, p.y), IOU_EPS);
    const float w2 = __fsub_rn(q.z, q.x), h2 = fmaxf(__fsub_rn(q.w, q.y), IOU_EPS);
    const float iw = fmaxf(0.f, __fsub_rn(fminf(p.z, q.z), fmaxf(p.x, q.x)));
    const float ih = fmaxf(0.f, __fsub_rn(fminf(p.w, q.w), fmaxf(p.y, q.y)));
    const float inter = __fmul_rn(iw, ih);
    const float uni = __fadd_rn(__fsub_rn(__fadd_rn(__fmul_rn(w1, h1), __fmul_rn(w2, h2)), inter), IOU_EPS);
    const float iou = __fdiv_rn(inter, uni);
    const float cw = __fsub_rn(fmaxf(p.z, q.z), fminf(p.x, q.x));
    const float ch = __fsub_rn(fmaxf(p.w, q.w), fminf(p.y, q.y));
    const float c2 = __fadd_rn(__fadd_rn(sq_rn(cw), sq_rn(ch)), IOU_EPS);
    const float dx = __fsub_rn(__fsub_rn(__fadd_rn(q.x, q.z), p.x), p.z);
    const float dy = __fsub_rn(__fsub_rn(__fadd_rn(q.y, q.w), p.y), p.w);
    const float rho2 = __fdiv_rn(__fadd_rn(sq_rn(dx), sq_rn(dy)), 4.f);
    const float v = __fmul_rn(CIOU_K, sq_rn(__fsub_rn(atanf(__fdiv_rn(w2, h2)), atanf(__fdiv_rn(w1, h1)))));
    const float alpha = __fdiv_rn(v, __fadd_rn(__fsub_rn(v, iou), ONE_EPS));
    return __fsub_rn(iou, __fadd_rn(__fdiv_rn(rho2, c2), __fmul_rn(v, alpha)));
}

// candidate v of image `img`: the output row [x1, y1, x2, y2, conf, cls] (:666-674) and the class-offset box NMS runs on (:692-693)
__device__ __forceinline__ void load_candidate(const NmsArgs &a, const float *img, uint32_t v, BoxO &me, float out6[6]) {
    const int row = (int)(v / (uint32_t)a.nc), cls = (int)(v % (uint32_t)a.nc);
    const float *p = img + (size_t)row * a.no;
    const float cx = p[0], cy = p[1], hw = __fdiv_rn(p[2], 2.f), hh = __fdiv_rn(p[3], 2.f);
    out6[0] = __fsub_rn(cx, hw);
    out6[1] = __fsub_rn(cy, hh);
    out6[2] = __fadd_rn(cx, hw);
    out6[3] = __fadd_rn(cy, hh);
    out6[4] = __fmul_rn(p[5 + cls], p[4]);
    out6[5] = (float)cls;
    const float c = a.agnostic ? 0.f : __fmul_rn((float)cls, MAX_WH);
    me.x1 = __fadd_rn(out6[0], c);
    me.y1 = __fadd_rn(out6[1], c);
    me.x2 = __fadd_rn(out6[2], c);
    me.y2 = __fadd_rn(out6[3], c);
    me.area = __fmul_rn(__fsub_rn(me.x2, me.x1), __fsub_rn(me.y2, me.y1));
}

// MODE: the overlap rule.  BOXES: candidates come from a.boxes (no class offset), kept indices go to a.keep, and the kept list, which
// has no max_det bound there, lives in global memory (a.kept_g) instead of LDS.
template <int MODE, bool BOXES>
__global__ __launch_bounds__(ROUND) void nms_greedy_kernel(const NmsArgs a, const uint32_t *sortV) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    BoxO *kept = BOXES ? a.kept_g : reinterpret_cast<BoxO *>(smem);      // [max_det]
    BoxO *cand = BOXES ? reinterpret_cast<BoxO *>(smem) : kept + a.max_det;   // [ROUND]
    uint32_t *mat = reinterpret_cast<uint32_t *>(cand + ROUND);          // [ROUND][ROUND/32] suppression bits (j > i)
    uint32_t *alive = mat + ROUND * (ROUND / 32);                        // [ROUND/32]
    __shared__ int nk_sh, nsel_sh;
    __shared__ int sel[ROUND];                                           // indices (within the round) kept this round
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    int n = a.total[b];
    if (n > MAX_NMS) n = MAX_NMS;
    const uint32_t *vals = sortV + (size_t)b * MAX_NMS;
    const float *img = a.pred + (size_t)b * a.n * a.no;
    float *det = a.det + (size_t)b * a.max_det * 6;
    if (tid == 0) nk_sh = 0;
    __syncthreads();
    for (int r0 = 0; r0 < n; r0 += ROUND) {
        const int nk = nk_sh;
        if (nk >= a.max_det) break;
        const int i = r0 + tid;
        const bool ok = i < n;
        BoxO me = {0.f, 0.f, 0.f, 0.f, 0.f};
        float out6[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        uint32_t v = 0;
        if (ok) {
            v = vals[i];
            if (BOXES) {
                const float4 q = reinterpret_cast<const float4 *>(a.boxes)[v];
                me.x1 = q.x; me.y1 = q.y; me.x2 = q.z; me.y2 = q.w;
                me.area = __fmul_rn(__fsub_rn(me.x2, me.x1), __fsub_rn(me.y2, me.y1));
            } else {
                load_candidate(a, img, v, me, out6);
            }
        }
        cand[tid] = me;
        // phase 1: suppressed by a box kept in an earlier round?
        bool live = ok;
        for (int k = 0; k < nk && live; ++k) live = !suppresses<MODE>(kept[k], me, a.iou_thres);
        const unsigned long long bal = __ballot(live);
        if (lane == 0) {
            alive[(tid >> 5)] = (uint32_t)bal;
            alive[(tid >> 5) + 1] = (uint32_t)(bal >> 32);
        }
        __syncthreads();
        // phase 2: this round's suppression matrix, row tid = bits j > tid with IoU > thr (only if both live)
        for (int w = 0; w < ROUND / 32; ++w) {
            uint32_t bits = 0;
            if (live && (w * 32 + 31) > tid) {
                const uint32_t al = alive[w];
                for (int jj = 0; jj < 32; ++jj) {
                    const int j = w * 32 + jj;
                    if (j > tid && ((al >> jj) & 1u) && suppresses<MODE>(me, cand[j], a.iou_thres)) bits |= 1u << jj;
                }
            }
            mat[tid * (ROUND / 32) + w] = bits;
        }
        __syncthreads();
        // phase 3: serial resolve in wave 0: lanes 0..15 each own one 32-bit word of the `removed` set
        if (tid < 64) {
            uint32_t removed = 0;                       // word `lane` (lanes >= 16 idle)
            int nsel = 0, room = a.max_det - nk;
            for (int i2 = 0; i2 < ROUND && nsel < room; ++i2) {
                const int w = i2 >> 5;
                const uint32_t aw = alive[w];
                const uint32_t rw = __shfl(removed, w);
                if (((aw >> (i2 & 31)) & 1u) && !((rw >> (i2 & 31)) & 1u)) {
                    if (lane == 0) sel[nsel] = i2;
                    ++nsel;
                    if (lane < ROUND / 32) removed |= mat[i2 * (ROUND / 32) + lane];
                }
            }
            if (lane == 0) nsel_sh = nsel;
        }
        __syncthreads();
        // phase 4: append survivors (in order) to the kept list and the output
        const int nsel = nsel_sh;
        // each thread checks whether it was selected: position = rank in sel[]
        if (ok) {
            // binary search of tid in sel[0..nsel)
            int lo = 0, hi = nsel;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (sel[mid] < tid) lo = mid + 1; else hi = mid;
            }
            if (lo < nsel && sel[lo] == tid) {
                const int slot = nk + lo;
                kept[slot] = me;
                if (BOXES) {
                    a.keep[slot] = (int64_t)v;
                } else {
#pragma unroll
                    for (int e = 0; e < 6; ++e) det[slot * 6 + e] = out6[e];
                }
            }
        }
        __syncthreads();
        if (tid == 0) nk_sh = nk + nsel;
        __syncthreads();
    }
    if (tid == 0) a.count[b] = nk_sh;
}

// ------------------------------------------------------------------------------------------------ Soft-NMS
// general.py:834-862 on the sorted candidates (the boxes + scores form takes them in the given order, like the reference).  One workgroup
// per image; the candidate state (offset box, score, live flag) sits in L2-resident global arrays, every candidate j is only ever touched
// by thread j % SOFT_T.  Per pick: keep `cur` with its score as it stands; one pass decays every live j by exp(-(m*m)/sigma) where
// m = CIoU(cur, j) > thr, drops it unless score > score_thres, and carries the running (max score, lowest index) pair; one block-wide
// reduction names the next `cur`.  At most max_det picks: a kept score is final when it is picked.  `hi` (one past the last live index)
// shrinks with the live set, which after the first pick is only what the score threshold left.  Unlike the reference's loop, which leaves
// with one candidate in hand and drops it, the last candidate is kept.
constexpr int SOFT_T = 1024;

template <bool BOXES>
__global__ __launch_bounds__(SOFT_T) void nms_soft_kernel(const NmsArgs a, const uint32_t *sortV, float4 *sbox_, float *sscore_,
                                                          uint8_t *slive_) {
    __shared__ float red_s[SOFT_T / 64];
    __shared__ int red_i[SOFT_T / 64], red_h[SOFT_T / 64];
    __shared__ int cur_sh, hi_sh;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int n = a.total[b];
    if (n > MAX_NMS) n = MAX_NMS;
    const uint32_t *vals = sortV + (size_t)b * MAX_NMS;
    const float *img = BOXES ? nullptr : a.pred + (size_t)b * a.n * a.no;
    float *det = BOXES ? nullptr : a.det + (size_t)b * a.max_det * 6;
    float4 *sbox = sbox_ + (size_t)b * MAX_NMS;
    float *sscore = sscore_ + (size_t)b * MAX_NMS;
    uint8_t *slive = slive_ + (size_t)b * MAX_NMS;
    for (int j = tid; j < n; j += SOFT_T) {
        const uint32_t v = vals[j];
        if (BOXES) {
            sbox[j] = reinterpret_cast<const float4 *>(a.boxes)[v];
            sscore[j] = a.scores[v];
        } else {
            BoxO me;
            float out6[6];
            load_candidate(a, img, v, me, out6);
            sbox[j] = make_float4(me.x1, me.y1, me.x2, me.y2);
            sscore[j] = out6[4];
        }
        slive[j] = 1;
    }
    __syncthreads();
    int cur = 0, hi = n, nk = 0;
    while (nk < n) {                                                     // n == 0: nothing to keep
        if (tid == 0) {
            const uint32_t v = vals[cur];
            if (BOXES) {
                a.keep[nk] = (int64_t)v;
            } else {
                BoxO me;
                float out6[6];
                load_candidate(a, img, v, me, out6);
                out6[4] = sscore[cur];                                   // the decayed score (the reference's scores view x[:, 4])
                for (int e = 0; e < 6; ++e) det[nk * 6 + e] = out6[e];
            }
            slive[cur] = 0;
        }
        ++nk;
        if (nk >= a.max_det) break;
        const float4 cb = sbox[cur];
        float best = 0.f;
        int bidx = 0x7fffffff, myhi = 0;
        for (int j = tid; j < hi; j += SOFT_T) {
            if (j == cur || !slive[j]) continue;
            const float m = ciou_for_soft_nms(cb, sbox[j]);
            float s = sscore[j];
            if (m > a.iou_thres) {
                s = __fmul_rn(s, expf(__fdiv_rn(-__fmul_rn(m, m), a.sigma)));
                sscore[j] = s;
            }
            if (!(s > a.score_thres)) {
                slive[j] = 0;
            } else {
                if (bidx == 0x7fffffff || s > best) { best = s; bidx = j; }   // j ascends: an exact tie stays with the lowest index
                myhi = j + 1;
            }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const float os = __shfl_xor(best, o);
            const int oi = __shfl_xor(bidx, o), oh = __shfl_xor(myhi, o);
            if (oi != 0x7fffffff && (bidx == 0x7fffffff || os > best || (os == best && oi < bidx))) { best = os; bidx = oi; }
            myhi = max(myhi, oh);
        }
        if (lane == 0) { red_s[wave] = best; red_i[wave] = bidx; red_h[wave] = myhi; }
        __syncthreads();
        if (tid == 0) {
            float bs = red_s[0];
            int bi = red_i[0], bh = red_h[0];
            for (int w = 1; w < SOFT_T / 64; ++w) {
                const float os = red_s[w];
                const int oi = red_i[w];
                if (oi != 0x7fffffff && (bi == 0x7fffffff || os > bs || (os == bs && oi < bi))) { bs = os; bi = oi; }
                bh = max(bh, red_h[w]);
            }
            cur_sh = bi;
            hi_sh = bh;
        }
        __syncthreads();
        cur = cur_sh;
        hi = hi_sh;
        if (cur == 0x7fffffff) break;                                    // nothing is live
    }
    if (BOXES) {                                                         // the reference decays `scores` in place (:851)
        __syncthreads();
        for (int j = tid; j < n; j += SOFT_T) a.scores[vals[j]] = sscore[j];
    }
    if (tid == 0) a.count[b] = nk;
}

// ------------------------------------------------------------------------------------------------ merge-NMS
// general.py:698-704, after the keep list is cut to max_det, for images with 1 < n < 3000 candidates.  One workgroup per kept box i:
// mask_j = box_iou(boxes[i], boxes[j]) > thr on the class-offset boxes (plain IoU, utils/metrics.py:234-235 = iou_gt's arithmetic,
// whatever rule selected), w_j = mask_j * score_j, box_i = sum_j w_j x_j[:4] / sum_j w_j on the un-offset boxes.  Thread t sums
// j = t, t + 256, ... in ascending order and the partial sums meet in a fixed tree, so two launches give the same bits.
// flag[b][i] = (sum_j mask_j > 1), the `redundant` test; nms_merge_compact_kernel then drops the unflagged rows in order.
__global__ __launch_bounds__(256) void nms_merge_kernel(const NmsArgs a, const uint32_t *sortV, int *flag) {
    __shared__ float red[4][5];
    __shared__ int redc[4];
    const int b = blockIdx.y, k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = a.total[b];
    if (!(n > 1 && n < 3000)) return;
    if (k >= a.count[b]) return;
    const uint32_t *vals = sortV + (size_t)b * MAX_NMS;
    const float *img = a.pred + (size_t)b * a.n * a.no;
    float *row = a.det + ((size_t)b * a.max_det + k) * 6;
    BoxO ki;
    {
        const float c = a.agnostic ? 0.f : __fmul_rn(row[5], MAX_WH);
        ki.x1 = __fadd_rn(row[0], c);
        ki.y1 = __fadd_rn(row[1], c);
        ki.x2 = __fadd_rn(row[2], c);
        ki.y2 = __fadd_rn(row[3], c);
        ki.area = __fmul_rn(__fsub_rn(ki.x2, ki.x1), __fsub_rn(ki.y2, ki.y1));
    }
    float s[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    int cnt = 0;
    for (int j = tid; j < n; j += 256) {
        BoxO cj;
        float o[6];
        load_candidate(a, img, vals[j], cj, o);
        if (iou_gt(ki, cj, a.iou_thres)) {
            ++cnt;
            s[4] += o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) s[e] += o[4] * o[e];
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int e = 0; e < 5; ++e) s[e] += __shfl_xor(s[e], o);
        cnt += __shfl_xor(cnt, o);
    }
    if (lane == 0) {
#pragma unroll
        for (int e = 0; e < 5; ++e) red[wave][e] = s[e];
        redc[wave] = cnt;
    }
    __syncthreads();                                                     // every thread has read its row by now
    if (tid < 4) {
        const float num = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
        const float den = (red[0][4] + red[1][4]) + (red[2][4] + red[3][4]);
        row[tid] = num / den;
    }
    if (tid == 0) flag[b * a.max_det + k] = (redc[0] + redc[1] + redc[2] + redc[3]) > 1 ? 1 : 0;
}

__global__ __launch_bounds__(MAX_DET_CAP) void nms_merge_compact_kernel(const NmsArgs a, const int *flag) {
    __shared__ int fl[MAX_DET_CAP];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = a.total[b];
    if (!(n > 1 && n < 3000)) return;
    const int nk = a.count[b];
    float *det = a.det + (size_t)b * a.max_det * 6;
    float r[6];
    const int f = tid < nk ? flag[b * a.max_det + tid] : 0;
    if (f)
        for (int e = 0; e < 6; ++e) r[e] = det[tid * 6 + e];
    fl[tid] = f;
    __syncthreads();
    int pos = 0;
    for (int t = 0; t < tid; ++t) pos += fl[t];
    __syncthreads();
    if (f)
        for (int e = 0; e < 6; ++e) det[pos * 6 + e] = r[e];
    if (tid == MAX_DET_CAP - 1) a.count[b] = pos + f;
}

// boxes + scores form: key = descending-order image of the score bits (any sign), val = index.  -0.0 takes the key of +0.0: the
// reference's sort compares them equal and leaves them in index order
__global__ void nms_boxes_prep_kernel(const NmsArgs a, uint32_t *sortV, int identity) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) a.total[0] = a.n;
    if (i >= a.n) return;
    if (identity) { sortV[i] = (uint32_t)i; return; }
    uint32_t u = __float_as_uint(a.scores[i]);
    if (u == 0x80000000u) u = 0u;
    a.keyA[i] = ~((u & 0x80000000u) ? ~u : (u | 0x80000000u));
    a.valA[i] = (uint32_t)i;
}

}  // namespace somi

using namespace somi;

extern "C" size_t somi_nms_workspace_bytes(int B, int n, int nc, int multi_label) {
    if (B <= 0 || n <= 0 || nc <= 0) return 0;
    const size_t nchunk = (size_t)(n + nms_chunk_rows(nc) - 1) / nms_chunk_rows(nc);
    const size_t cap = (size_t)n * (size_t)((multi_label && nc > 1) ? nc : 1);
    const size_t nsel_chunk = (cap + SEL_CHUNK - 1) / SEL_CHUNK;
    return align_up((size_t)B * nchunk * 4, 256) * 2 + align_up((size_t)B * 4, 256) + align_up((size_t)B * cap * 4, 256) * 4 +
           align_up((size_t)B * sizeof(SelState), 256) + align_up((size_t)B * nsel_chunk * sizeof(int2), 256) +
           align_up((size_t)B * MAX_NMS * 4, 256);
}

static size_t nms_workspace(int B, int n, int nc, int multi_label, int mode, int merge) {
    size_t bytes = somi_nms_workspace_bytes(B, n, nc, multi_label);
    if (!bytes) return 0;
    if (mode == NMS_SOFT)
        bytes += align_up((size_t)B * MAX_NMS * sizeof(float4), 256) + align_up((size_t)B * MAX_NMS * 4, 256) + align_up((size_t)B * MAX_NMS, 256);
    if (merge) bytes += align_up((size_t)B * MAX_DET_CAP * 4, 256);
    return bytes;
}

static int nms_run(const char *who, const float *pred, int B, int n, int nc, float conf_thres, float iou_thres, int multi_label, int agnostic,
                   const uint64_t *classes_mask, int max_det, int mode, int merge, float sigma, float score_thres, float *det, int32_t *count,
                   void *workspace, size_t workspace_bytes, somi_stream_t stream) {
    SOMI_REQUIRE(pred && det && count && workspace, SOMI_EINVAL, "nms: null tensor");
    SOMI_REQUIRE(B > 0 && n > 0 && nc > 0 && nc <= 64 * NMS_MASK_WORDS, SOMI_EINVAL, "nms: bad sizes (nc <= %d)", 64 * NMS_MASK_WORDS);
    SOMI_REQUIRE(conf_thres >= 0.f && conf_thres <= 1.f, SOMI_EINVAL,
                 "Invalid Confidence threshold %g, valid values are between 0.0 and 1.0", conf_thres);   // general.py:635
    SOMI_REQUIRE(iou_thres >= 0.f && iou_thres <= 1.f, SOMI_EINVAL, "Invalid IoU %g, valid values are between 0.0 and 1.0",
                 iou_thres);                                                                             // general.py:636
    SOMI_REQUIRE(max_det > 0 && max_det <= MAX_DET_CAP, SOMI_EINVAL, "nms: max_det must be in [1, %d]", MAX_DET_CAP);
    SOMI_REQUIRE((size_t)n * nc < (1ull << 32), SOMI_EINVAL, "nms: n*nc must fit 32 bits");
    multi_label = (multi_label && nc > 1) ? 1 : 0;                                                       // general.py:643
    SOMI_REQUIRE(workspace_bytes >= nms_workspace(B, n, nc, multi_label, mode, merge), SOMI_EWORKSPACE, "nms: workspace too small");
    NmsArgs a = {};
    a.sigma = sigma; a.score_thres = score_thres;
    a.pred = pred; a.B = B; a.n = n; a.nc = nc; a.no = nc + 5;
    a.conf_thres = conf_thres; a.iou_thres = iou_thres; a.multi_label = multi_label; a.agnostic = agnostic;
    a.max_det = max_det;
    for (int i = 0; i < NMS_MASK_WORDS; ++i)                     // host words, NULL = keep every class (general.py:676-677)
        a.classes_mask[i] = classes_mask ? (i < (nc + 63) / 64 ? classes_mask[i] : 0ull) : ~0ull;
    a.nchunk = (n + nms_chunk_rows(nc) - 1) / nms_chunk_rows(nc);
    a.cap = n * (multi_label ? nc : 1);
    char *w = static_cast<char *>(workspace);
    const size_t s_chunk = align_up((size_t)B * a.nchunk * 4, 256), s_tot = align_up((size_t)B * 4, 256);
    const size_t s_buf = align_up((size_t)B * a.cap * 4, 256);
    a.chunk_cnt = reinterpret_cast<int *>(w); w += s_chunk;
    a.chunk_off = reinterpret_cast<int *>(w); w += s_chunk;
    a.total = reinterpret_cast<int *>(w); w += s_tot;
    a.keyA = reinterpret_cast<uint32_t *>(w); w += s_buf;
    a.valA = reinterpret_cast<uint32_t *>(w); w += s_buf;
    a.keyB = reinterpret_cast<uint32_t *>(w); w += s_buf;
    a.valB = reinterpret_cast<uint32_t *>(w); w += s_buf;
    const int nsel_chunk = (a.cap + SEL_CHUNK - 1) / SEL_CHUNK;
    SelState *st = reinterpret_cast<SelState *>(w); w += align_up((size_t)B * sizeof(SelState), 256);
    int2 *sel_cnt = reinterpret_cast<int2 *>(w); w += align_up((size_t)B * nsel_chunk * sizeof(int2), 256);
    uint32_t *sortV = reinterpret_cast<uint32_t *>(w);
    a.det = det; a.count = count;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (nms_chunk_rows(nc) == NMS_CHUNK) launch_count_emit<NMS_CHUNK / 256, true>(a, s);
    else if (nms_rows_staged(nc)) launch_count_emit<1, true>(a, s);
    else launch_count_emit<1, false>(a, s);
    // top-30000 select (every kernel exits at once for images with <= 30000 candidates)
    (void)hipMemsetAsync(st, 0, (size_t)B * sizeof(SelState), s);
    hipLaunchKernelGGL(nms_select_hist_kernel<1>, dim3(nsel_chunk, B), dim3(256), 0, s, a, st);
    hipLaunchKernelGGL(nms_select_hist_kernel<2>, dim3(nsel_chunk, B), dim3(256), 0, s, a, st);
    hipLaunchKernelGGL(nms_select_hist_kernel<3>, dim3(nsel_chunk, B), dim3(256), 0, s, a, st);
    hipLaunchKernelGGL(nms_select_compact_kernel<false>, dim3(nsel_chunk, B), dim3(256), 0, s, a, st, sel_cnt, nsel_chunk);
    hipLaunchKernelGGL(nms_select_scan_kernel, dim3(B), dim3(256), 0, s, a, sel_cnt, nsel_chunk);
    hipLaunchKernelGGL(nms_select_compact_kernel<true>, dim3(nsel_chunk, B), dim3(256), 0, s, a, st, sel_cnt, nsel_chunk);
    hipLaunchKernelGGL(nms_rank_sort_kernel, dim3((MAX_NMS + 255) / 256, B), dim3(256), 0, s, a, sortV);
    const size_t lds = (size_t)(max_det + ROUND) * sizeof(BoxO) + (size_t)ROUND * (ROUND / 32) * 4 + (ROUND / 32 + 2) * 4;
    w += align_up((size_t)B * MAX_NMS * 4, 256);
    if (mode == NMS_SOFT) {
        float4 *sbox = reinterpret_cast<float4 *>(w); w += align_up((size_t)B * MAX_NMS * sizeof(float4), 256);
        float *sscore = reinterpret_cast<float *>(w); w += align_up((size_t)B * MAX_NMS * 4, 256);
        uint8_t *slive = reinterpret_cast<uint8_t *>(w); w += align_up((size_t)B * MAX_NMS, 256);
        hipLaunchKernelGGL(nms_soft_kernel<false>, dim3(B), dim3(SOFT_T), 0, s, a, sortV, sbox, sscore, slive);
        return launch_status(who);
    }
    switch (mode) {
    case NMS_IOU: hipLaunchKernelGGL((nms_greedy_kernel<NMS_IOU, false>), dim3(B), dim3(ROUND), lds, s, a, sortV); break;
    case NMS_GIOU: hipLaunchKernelGGL((nms_greedy_kernel<NMS_GIOU, false>), dim3(B), dim3(ROUND), lds, s, a, sortV); break;
    case NMS_DIOU: hipLaunchKernelGGL((nms_greedy_kernel<NMS_DIOU, false>), dim3(B), dim3(ROUND), lds, s, a, sortV); break;
    case NMS_CIOU: hipLaunchKernelGGL((nms_greedy_kernel<NMS_CIOU, false>), dim3(B), dim3(ROUND), lds, s, a, sortV); break;
    case NMS_EIOU: hipLaunchKernelGGL((nms_greedy_kernel<NMS_EIOU, false>), dim3(B), dim3(ROUND), lds, s, a, sortV); break;
    default: hipLaunchKernelGGL((nms_greedy_kernel<NMS_SIOU, false>), dim3(B), dim3(ROUND), lds, s, a, sortV); break;
    }
    if (merge) {
        int *flag = reinterpret_cast<int *>(w);
        hipLaunchKernelGGL(nms_merge_kernel, dim3(max_det, B), dim3(256), 0, s, a, sortV, flag);
        hipLaunchKernelGGL(nms_merge_compact_kernel, dim3(B), dim3(MAX_DET_CAP), 0, s, a, flag);
    }
    return launch_status(who);
}

extern "C" int somi_nms_f32(const float *pred, int B, int n, int nc, float conf_thres, float iou_thres, int multi_label,
                            int agnostic, const uint64_t *classes_mask, int max_det, float *det, int32_t *count, void *workspace,
                            size_t workspace_bytes, somi_stream_t stream) {
    return nms_run("somi_nms_f32", pred, B, n, nc, conf_thres, iou_thres, multi_label, agnostic, classes_mask, max_det, NMS_IOU, 0, 0.5f, 0.25f,
                   det, count, workspace, workspace_bytes, stream);
}

extern "C" size_t somi_nms_ex_workspace_bytes(int B, int n, int nc, int multi_label, int mode, int merge) {
    return nms_workspace(B, n, nc, (multi_label && nc > 1) ? 1 : 0, mode, merge);
}

extern "C" int somi_nms_ex_f32(const float *pred, int B, int n, int nc, float conf_thres, float iou_thres, int multi_label, int agnostic,
                               const uint64_t *classes_mask, int max_det, int mode, int merge, float sigma, float score_threshold, float *det,
                               int32_t *count, void *workspace, size_t workspace_bytes, somi_stream_t stream) {
    SOMI_REQUIRE(mode >= 0 && mode < NMS_MODES, SOMI_EINVAL, "nms: unknown mode %d", mode);
    SOMI_REQUIRE(!(merge && mode == NMS_SOFT), SOMI_EINVAL, "nms: merge-NMS is not defined on Soft-NMS output");
    SOMI_REQUIRE(mode != NMS_SOFT || sigma > 0.f, SOMI_EINVAL, "nms: sigma must be positive");
    return nms_run("somi_nms_ex_f32", pred, B, n, nc, conf_thres, iou_thres, multi_label, agnostic, classes_mask, max_det, mode, merge ? 1 : 0,
                   sigma, score_threshold, det, count, workspace, workspace_bytes, stream);
}

extern "C" size_t somi_nms_boxes_workspace_bytes(int n) {
    if (n <= 0) return 0;
    return 256 + align_up((size_t)n * 4, 256) * 2 + align_up((size_t)MAX_NMS * 4, 256) + align_up((size_t)n * sizeof(BoxO), 256) +
           align_up((size_t)n * sizeof(float4), 256) + align_up((size_t)n * 4, 256) + align_up((size_t)n, 256);
}

extern "C" int somi_nms_boxes_f32(const float *boxes, float *scores, int n, int mode, float iou_thres, float sigma, float score_threshold,
                                  int64_t *keep, int32_t *count, void *workspace, size_t workspace_bytes, somi_stream_t stream) {
    SOMI_REQUIRE(boxes && scores && keep && count && workspace, SOMI_EINVAL, "nms_boxes: null tensor");
    SOMI_REQUIRE(n > 0 && n <= MAX_NMS, SOMI_EINVAL, "nms_boxes: n must be in [1, %d]", MAX_NMS);
    SOMI_REQUIRE(mode >= 0 && mode < NMS_MODES, SOMI_EINVAL, "nms_boxes: unknown mode %d", mode);
    SOMI_REQUIRE(mode != NMS_SOFT || sigma > 0.f, SOMI_EINVAL, "nms_boxes: sigma must be positive");
    SOMI_REQUIRE((reinterpret_cast<uintptr_t>(boxes) & 15u) == 0, SOMI_EINVAL, "nms_boxes: boxes must be 16-byte aligned");
    SOMI_REQUIRE(workspace_bytes >= somi_nms_boxes_workspace_bytes(n), SOMI_EWORKSPACE, "nms_boxes: workspace too small");
    NmsArgs a = {};
    a.B = 1; a.n = n; a.nc = 1; a.no = 6; a.cap = n; a.max_det = n;
    a.iou_thres = iou_thres; a.sigma = sigma; a.score_thres = score_threshold;
    a.boxes = boxes; a.scores = scores; a.keep = keep; a.count = count;
    char *w = static_cast<char *>(workspace);
    a.total = reinterpret_cast<int *>(w); w += 256;
    a.keyA = reinterpret_cast<uint32_t *>(w); w += align_up((size_t)n * 4, 256);
    a.valA = reinterpret_cast<uint32_t *>(w); w += align_up((size_t)n * 4, 256);
    uint32_t *sortV = reinterpret_cast<uint32_t *>(w); w += align_up((size_t)MAX_NMS * 4, 256);
    a.kept_g = reinterpret_cast<BoxO *>(w); w += align_up((size_t)n * sizeof(BoxO), 256);
    float4 *sbox = reinterpret_cast<float4 *>(w); w += align_up((size_t)n * sizeof(float4), 256);
    float *sscore = reinterpret_cast<float *>(w); w += align_up((size_t)n * 4, 256);
    uint8_t *slive = reinterpret_cast<uint8_t *>(w);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(nms_boxes_prep_kernel, dim3((n + 255) / 256), dim3(256), 0, s, a, sortV, mode == NMS_SOFT ? 1 : 0);
    if (mode == NMS_SOFT) {                                      // candidates in the given order, first pick index 0 (general.py:835,843)
        hipLaunchKernelGGL(nms_soft_kernel<true>, dim3(1), dim3(SOFT_T), 0, s, a, sortV, sbox, sscore, slive);
        return launch_status("somi_nms_boxes_f32");
    }
    hipLaunchKernelGGL(nms_rank_sort_kernel, dim3((n + 255) / 256, 1), dim3(256), 0, s, a, sortV);
    const size_t lds = (size_t)ROUND * sizeof(BoxO) + (size_t)ROUND * (ROUND / 32) * 4 + (ROUND / 32 + 2) * 4;
    switch (mode) {
    case NMS_IOU: hipLaunchKernelGGL((nms_greedy_kernel<NMS_IOU, true>), dim3(1), dim3(ROUND), lds, s, a, sortV); break;
    case NMS_GIOU: hipLaunchKernelGGL((nms_greedy_kernel<NMS_GIOU, true>), dim3(1), dim3(ROUND), lds, s, a, sortV); break;
    case NMS_DIOU: hipLaunchKernelGGL((nms_greedy_kernel<NMS_DIOU, true>), dim3(1), dim3(ROUND), lds, s, a, sortV); break;
    case NMS_CIOU: hipLaunchKernelGGL((nms_greedy_kernel<NMS_CIOU, true>), dim3(1), dim3(ROUND), lds, s, a, sortV); break;
    case NMS_EIOU: hipLaunchKernelGGL((nms_greedy_kernel<NMS_EIOU, true>), dim3(1), dim3(ROUND), lds, s, a, sortV); break;
    default: hipLaunchKernelGGL((nms_greedy_kernel<NMS_SIOU, true>), dim3(1), dim3(ROUND), lds, s, a, sortV); break;
    }
    return launch_status("somi_nms_boxes_f32");
}
