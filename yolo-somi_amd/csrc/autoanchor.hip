// AutoAnchor on the device (utils/autoanchor.py): the anchor metric (best possible recall, anchors above threshold, fitness), the genetic evolution of
// the anchors and the Lloyd iterations of scipy.cluster.vq.kmeans, batched over its restarts.
//
// Metric: per label best = max_k min(w / kw, kw / w, h / kh, kh / h) in fp32 with IEEE division for `wh / k` and `1 / r`, as torch computes it on the CPU
// (hipcc's default fp32 divide is the correctly rounded one; this file is built without any fast-math flag and with contraction off, see below).
// Every sum is taken in fp64 over terms that are 0 / 1 (the two counts) or an fp32 value in (thr, 1] (the fitness): for thr >= 1/8 each term is a
// multiple of 2^-26, so the fp64 sum over n < 2^27 labels is EXACT whatever the order.  The result does not depend on the grid shape or the reduction
// tree, and `fg > f` in the evolution compares two exact sums over the same labels.
//
// Evolution: k (fp64, na x 2), its fitness sum f and the table of mutation factors live on the device.  Generation g evaluates
// kg = max(k * v_g, 2.0) (fp64, rounded to fp32 for the metric like torch.tensor(kg, dtype=float32)) with one grid over the labels, and a one-block
// finishing kernel folds the partial sums, compares and commits k, f and the accepted-generation list.  Nothing returns to the host in between.
//
// k-means: fp64 like scipy's _vq (an fp32 Lloyd does not follow it).  One launch assigns every observation of every running restart to its nearest
// live code (squared distance summed feature by feature, first minimum wins, as _vq_small_nf) and leaves per-block partial sums; a second launch folds
// them in block order, moves the codes, drops codes without members and raises the restart's `done` flag when the mean distance moved by <= thresh.
// No float atomics anywhere: every sum has one fixed order per (n, k), so runs are bit-identical.
#include "common.h"

// a * b + c must stay two roundings: the CPU code this follows (scipy's _vq, numpy, torch) does not fuse
#pragma clang fp contract(off)

namespace somi {

constexpr int kAnchorMax = 64;       // anchors per metric call (LDS table)
constexpr int kMetricThreads = 256;
constexpr int kMetricMaxBlocks = 1024;
constexpr int kKmeansMaxK = 32;      // codes per restart: 20 bytes of LDS per (code, thread)
constexpr int kKmeansThreads = 64;
constexpr int kKmeansMaxBlocks = 128;
constexpr int kKmeansPad = kKmeansThreads + 1;

static inline int metric_blocks(long n) {
    long g = (n + kMetricThreads - 1) / kMetricThreads;
    return (int)(g < 1 ? 1 : (g > kMetricMaxBlocks ? kMetricMaxBlocks : g));
}

static inline int kmeans_blocks(long n) {
    long g = (n + kKmeansThreads * 8 - 1) / (kKmeansThreads * 8);
    return (int)(g < 1 ? 1 : (g > kKmeansMaxBlocks ? kKmeansMaxBlocks : g));
}

// fixed-order tree over the block's 256 values of three sums; the result is in s[0][*]
__device__ __forceinline__ void block_sum3(double (&s)[3][kMetricThreads], double a, double b, double c) {
    const int t = threadIdx.x;
    s[0][t] = a, s[1][t] = b, s[2][t] = c;
    __syncthreads();
    for (int w = kMetricThreads / 2; w > 0; w >>= 1) {
        if (t < w) {
            s[0][t] += s[0][t + w];
            s[1][t] += s[1][t + w];
            s[2][t] += s[2][t + w];
        }
        __syncthreads();
    }
}

// anchors: fp32 (na, 2) as given, or - when k64 is set - max(k64 * v, 2.0) rounded to fp32 (v may be null: factor 1).  partial: (gridDim.x, 3) =
// labels with best > thr, (label, anchor) pairs with x > thr, sum of best over the labels with best > thr.
__global__ __launch_bounds__(kMetricThreads) void anchor_metric_kernel(const float *__restrict__ wh, long n, const float *__restrict__ anchors,
                                                                       const double *__restrict__ k64, const double *__restrict__ v, int na, float thr,
                                                                       float *__restrict__ best_out, double *__restrict__ partial) {
    __shared__ float a[kAnchorMax * 2];
    __shared__ double red[3][kMetricThreads];
    const int t = threadIdx.x;
    if (t < na * 2) {
        if (k64) {
            double kg = v ? k64[t] * v[t] : k64[t];
            if (v && kg < 2.0) kg = 2.0;
            a[t] = (float)kg;
        } else {
            a[t] = anchors[t];
        }
    }
    __syncthreads();
    double n_best = 0.0, n_x = 0.0, fit = 0.0;
    for (long i = (long)blockIdx.x * kMetricThreads + t; i < n; i += (long)gridDim.x * kMetricThreads) {
        const float w = wh[2 * i], h = wh[2 * i + 1];
        float best = 0.f;
        int cnt = 0;
        for (int j = 0; j < na; ++j) {
            const float rw = w / a[2 * j], rh = h / a[2 * j + 1];
            const float xw = fminf(rw, 1.0f / rw), xh = fminf(rh, 1.0f / rh);
            const float x = fminf(xw, xh);
            cnt += x > thr;
            best = (j == 0 || x > best) ? x : best;
        }
        if (best_out) best_out[i] = best;
        n_x += (double)cnt;
        if (best > thr) {
            n_best += 1.0;
            fit += (double)best;
        }
    }
    block_sum3(red, n_best, n_x, fit);
    if (t == 0) {
        partial[blockIdx.x * 3 + 0] = red[0][0];
        partial[blockIdx.x * 3 + 1] = red[1][0];
        partial[blockIdx.x * 3 + 2] = red[2][0];
    }
}

__device__ __forceinline__ void fold_partials(double (&red)[3][kMetricThreads], const double *__restrict__ partial, int nblk) {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int b = threadIdx.x; b < nblk; b += kMetricThreads) {
        s0 += partial[b * 3 + 0];
        s1 += partial[b * 3 + 1];
        s2 += partial[b * 3 + 2];
    }
    block_sum3(red, s0, s1, s2);
}

__global__ __launch_bounds__(kMetricThreads) void anchor_metric_fold_kernel(const double *__restrict__ partial, int nblk, double *__restrict__ out) {
    __shared__ double red[3][kMetricThreads];
    fold_partials(red, partial, nblk);
    if (threadIdx.x < 3) out[threadIdx.x] = red[threadIdx.x][0];
}

// the finishing step of generation g: if the candidate's fitness sum beats f, k <- max(k * v, 2.0), f <- fg and g joins the accepted list
// (accepted[0] = count, accepted[1..] = generations in order)
__global__ __launch_bounds__(kMetricThreads) void anchor_commit_kernel(const double *__restrict__ partial, int nblk, double *__restrict__ k,
                                                                       const double *__restrict__ v, int na, double *__restrict__ f,
                                                                       int32_t *__restrict__ accepted, int g) {
    __shared__ double red[3][kMetricThreads];
    const int t = threadIdx.x;
    const double f_old = *f;
    fold_partials(red, partial, nblk);       // ends with a barrier: every thread has read f before thread 0 writes it
    const double fg = red[2][0];
    if (!(fg > f_old)) return;
    if (t < na * 2) {
        const double kg = k[t] * v[t];
        k[t] = kg < 2.0 ? 2.0 : kg;
    }
    if (t == 0) {
        *f = fg;
        const int c = accepted[0];
        accepted[1 + c] = g;
        accepted[0] = c + 1;
    }
}

// ---------------------------------------------------------------------------------------------------------------- k-means
// grid (blocks, restarts).  partial: (restarts, blocks, K * 3 + 1) = per code sum x, sum y, members; then the sum of the distances to the nearest code.
__global__ __launch_bounds__(kKmeansThreads) void kmeans_assign_kernel(const double *__restrict__ obs, long n, const double *__restrict__ book,
                                                                       const int32_t *__restrict__ alive, const int32_t *__restrict__ done, int K,
                                                                       double *__restrict__ partial) {
    extern __shared__ double lds[];
    const int r = blockIdx.y, t = threadIdx.x;
    if (done[r]) return;
    double *sx = lds, *sy = sx + K * kKmeansPad, *bk = sy + K * kKmeansPad, *ds = bk + K * 2;
    int32_t *cn = reinterpret_cast<int32_t *>(ds + kKmeansThreads), *al = cn + K * kKmeansPad;
    for (int j = t; j < K; j += kKmeansThreads) {
        bk[2 * j] = book[((long)r * K + j) * 2];
        bk[2 * j + 1] = book[((long)r * K + j) * 2 + 1];
        al[j] = alive[r * K + j];
    }
    for (int j = 0; j < K; ++j) sx[j * kKmeansPad + t] = 0.0, sy[j * kKmeansPad + t] = 0.0, cn[j * kKmeansPad + t] = 0;
    __syncthreads();
    double dsum = 0.0;
    for (long i = (long)blockIdx.x * kKmeansThreads + t; i < n; i += (long)gridDim.x * kKmeansThreads) {
        const double x = obs[2 * i], y = obs[2 * i + 1];
        double low = __builtin_huge_val();
        int code = -1;
        for (int j = 0; j < K; ++j) {
            if (!al[j]) continue;
            const double dx = bk[2 * j] - x, dy = bk[2 * j + 1] - y;
            double d = dx * dx;
            d += dy * dy;
            if (d < low) low = d, code = j;
        }
        if (code >= 0) {
            dsum += __dsqrt_rn(low);
            sx[code * kKmeansPad + t] += x;
            sy[code * kKmeansPad + t] += y;
            cn[code * kKmeansPad + t] += 1;
        }
    }
    ds[t] = dsum;
    __syncthreads();
    double *out = partial + ((long)r * gridDim.x + blockIdx.x) * (K * 3 + 1);
    for (int j = t; j < K; j += kKmeansThreads) {
        double ax = 0.0, ay = 0.0;
        long ac = 0;
        for (int q = 0; q < kKmeansThreads; ++q) ax += sx[j * kKmeansPad + q], ay += sy[j * kKmeansPad + q], ac += cn[j * kKmeansPad + q];
        out[j * 3 + 0] = ax, out[j * 3 + 1] = ay, out[j * 3 + 2] = (double)ac;
    }
    if (t == 0) {
        double a = 0.0;
        for (int q = 0; q < kKmeansThreads; ++q) a += ds[q];
        out[K * 3] = a;
    }
}

// one block per restart: new codes = member sums / member counts (update_cluster_means), codes without members leave the book, dist = mean distance of
// THIS assignment (what _kmeans returns next to the moved book), done when |previous mean - this mean| <= thresh
__global__ __launch_bounds__(kKmeansThreads) void kmeans_update_kernel(const double *__restrict__ partial, int nblk, long n, double *__restrict__ book,
                                                                       int32_t *__restrict__ alive, int K, double thresh, double *__restrict__ dist,
                                                                       int32_t *__restrict__ done, int32_t *__restrict__ iters) {
    const int r = blockIdx.x, t = threadIdx.x;
    const int was_done = done[r];
    __syncthreads();
    if (was_done) return;
    const double *p = partial + (long)r * nblk * (K * 3 + 1);
    for (int j = t; j < K; j += kKmeansThreads) {
        double ax = 0.0, ay = 0.0, ac = 0.0;
        for (int b = 0; b < nblk; ++b) {
            const double *q = p + (long)b * (K * 3 + 1) + j * 3;
            ax += q[0], ay += q[1], ac += q[2];
        }
        if (alive[r * K + j]) {
            if (ac > 0.0) {
                book[((long)r * K + j) * 2] = ax / ac;
                book[((long)r * K + j) * 2 + 1] = ay / ac;
            } else {
                alive[r * K + j] = 0;
            }
        }
    }
    if (t == 0) {
        double a = 0.0;
        for (int b = 0; b < nblk; ++b) a += p[(long)b * (K * 3 + 1) + K * 3];
        const double avg = a / (double)n;
        const double diff = fabs(dist[r] - avg);
        dist[r] = avg;
        iters[r] += 1;
        if (!(diff > thresh)) done[r] = 1;
    }
}

static size_t kmeans_lds_bytes(int K) {
    return (size_t)(2 * K * kKmeansPad + 2 * K + kKmeansThreads) * sizeof(double) + (size_t)(K * kKmeansPad + K) * sizeof(int32_t);
}

}  // namespace somi

using namespace somi;

extern "C" size_t somi_anchor_metric_workspace_bytes(long n) { return n < 0 ? 0 : (size_t)metric_blocks(n) * 3 * sizeof(double); }

extern "C" int somi_anchor_metric_f32(const float *wh, long n, const float *anchors, int na, float thr, float *best, double *out, void *workspace,
                                      size_t workspace_bytes, somi_stream_t stream) {
    SOMI_REQUIRE(wh && anchors && out && workspace && n > 0 && n < (1L << 27), SOMI_EINVAL, "anchor metric: bad arguments (1 <= n < 2^27 labels)");
    SOMI_REQUIRE(na >= 1 && na <= kAnchorMax, SOMI_EINVAL, "anchor metric: 1 to %d anchors", kAnchorMax);
    SOMI_REQUIRE(workspace_bytes >= somi_anchor_metric_workspace_bytes(n), SOMI_EINVAL, "anchor metric: workspace too small");
    const int nblk = metric_blocks(n);
    hipLaunchKernelGGL(anchor_metric_kernel, dim3(nblk), dim3(kMetricThreads), 0, (hipStream_t)stream, wh, n, anchors, (const double *)nullptr,
                       (const double *)nullptr, na, thr, best, (double *)workspace);
    hipLaunchKernelGGL(anchor_metric_fold_kernel, dim3(1), dim3(kMetricThreads), 0, (hipStream_t)stream, (const double *)workspace, nblk, out);
    return launch_status("somi_anchor_metric_f32");
}

extern "C" int somi_anchor_evolve_f32(const float *wh, long n, double *k, int na, const double *v, int gen, float thr, double *fitness,
                                      int32_t *accepted, void *workspace, size_t workspace_bytes, somi_stream_t stream) {
    SOMI_REQUIRE(wh && k && fitness && accepted && workspace && n > 0 && n < (1L << 27), SOMI_EINVAL,
                 "anchor evolve: bad arguments (1 <= n < 2^27 labels)");
    SOMI_REQUIRE(na >= 1 && na <= kAnchorMax && gen >= 0 && (v || gen == 0), SOMI_EINVAL, "anchor evolve: 1 to %d anchors, gen >= 0", kAnchorMax);
    SOMI_REQUIRE(workspace_bytes >= somi_anchor_metric_workspace_bytes(n), SOMI_EINVAL, "anchor evolve: workspace too small");
    const int nblk = metric_blocks(n);
    hipStream_t s = (hipStream_t)stream;
    for (int g = 0; g < gen; ++g) {
        const double *vg = v + (long)g * na * 2;
        hipLaunchKernelGGL(anchor_metric_kernel, dim3(nblk), dim3(kMetricThreads), 0, s, wh, n, (const float *)nullptr, (const double *)k, vg, na, thr,
                           (float *)nullptr, (double *)workspace);
        hipLaunchKernelGGL(anchor_commit_kernel, dim3(1), dim3(kMetricThreads), 0, s, (const double *)workspace, nblk, k, vg, na, fitness, accepted, g);
    }
    return launch_status("somi_anchor_evolve_f32");
}

extern "C" size_t somi_kmeans_workspace_bytes(long n, int k, int restarts) {
    if (n < 0 || k < 1 || restarts < 1) return 0;
    return (size_t)restarts * kmeans_blocks(n) * (k * 3 + 1) * sizeof(double);
}

extern "C" int somi_kmeans_lloyd_step_f64(const double *obs, long n, double *book, int32_t *alive, int k, int restarts, double thresh, double *dist,
                                          int32_t *done, int32_t *iters, void *workspace, size_t workspace_bytes, somi_stream_t stream) {
    SOMI_REQUIRE(obs && book && alive && dist && done && iters && workspace && n > 0 && n < (1L << 31), SOMI_EINVAL, "kmeans: bad arguments");
    SOMI_REQUIRE(k >= 1 && k <= kKmeansMaxK && restarts >= 1 && restarts <= 65535, SOMI_EINVAL, "kmeans: 1 to %d codes, 1 to 65535 restarts",
                 kKmeansMaxK);
    SOMI_REQUIRE(workspace_bytes >= somi_kmeans_workspace_bytes(n, k, restarts), SOMI_EINVAL, "kmeans: workspace too small");
    const int nblk = kmeans_blocks(n);
    hipLaunchKernelGGL(kmeans_assign_kernel, dim3(nblk, restarts), dim3(kKmeansThreads), kmeans_lds_bytes(k), (hipStream_t)stream, obs, n,
                       (const double *)book, (const int32_t *)alive, (const int32_t *)done, k, (double *)workspace);
    hipLaunchKernelGGL(kmeans_update_kernel, dim3(restarts), dim3(kKmeansThreads), 0, (hipStream_t)stream, (const double *)workspace, nblk, n, book,
                       alive, k, thresh, dist, done, iters);
    return launch_status("somi_kmeans_lloyd_step_f64");
}
