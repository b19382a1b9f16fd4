// SimAM attention (SimAM, models/common.py:2915-2939; SimAMWithSlicing, :9374-9408; SimAMWithFlexibleSlicing, :9411-9480): one operator over a
// grid of ny x nx regions of the (B,H,W,C) map.  Region (i, j) spans rows [i * step_y, i * step_y + len_y) and columns likewise; with stretch_last
// the last region of an axis runs to the map edge (the quadrants of an odd map).  Per (image, region r, channel), N_r the region's pixel count:
//   mu_r = mean of x over r,  d = x - mu_r,  S_r = sum d^2,  D_r = 4 (S_r / n + lambda),  s = sigmoid(d^2 / D_r + 0.5)
//   out  = [x +] sum_{r covers the pixel} w x s,   w = 1 / k,  k = the pixel's 1-based rank of r among the regions that cover it, row-major
// (the reference divides a window's contribution by the coverage count at the time it is added).  A pixel no region covers gets 0 [+ x].
//   stats      stats[b][r][0][c] = mu_r, stats[b][r][1][c] = S_r                               reads x
//   apply      out                                                                           reads x, stats
//   bwd sums   sums[b][r][0][c] = A_r = sum T d, sums[b][r][1][c] = B_r = sum T d^2,  T = w g x s (1 - s)      reads dout, x, stats
//   bwd input  dx = [dx +] [g +] sum_r ( w g s + 2 T d / D_r - 2 A_r / (N_r D_r) - (8 / n) d B_r / D_r^2 )      reads dout, x, stats, sums
//
// The two reductions share one geometry: a workgroup of 256 = NL pixel lanes x QW channel quads takes a band of RB regions in a row and, of each,
// the pixel chunk blockIdx.x: SA_K * NL pixels, lane l the pixels l, l + NL, ... of the chunk in the region's row-major order.  A lane holds its
// SA_K values in registers: its mean, then its sum of squared deviations ABOUT that mean - never sum x^2 - N mu^2, which cancels on maps with an
// offset.  Lanes are merged through LDS by a fixed tree with the pairwise update (count, mean, M2); a region larger than one chunk leaves
// (mean, M2) per chunk in the caller's workspace and a second launch merges the chunks in order.  The backward sums take the same route with
// plain additions.  Few large regions get their parallelism from the pixel chunks, many small ones from the bands.  No float atomics: two
// launches are bit-identical.
#include "common.h"

namespace somi {

constexpr int SA_K = 8;           // pixels a lane holds in registers: a chunk is SA_K * NL pixels
constexpr int SA_COVER = 4;       // at most this many regions cover a pixel along one axis

struct SaGeom {
    int H, W, C4, ny, nx, sy, sx, ly, lx, stretch;
    float inv_n, lambda;
};

struct SaPlan {
    int QW, NL, nQc, nP, RB, R;   // quads and pixel lanes of a workgroup, quad chunks, pixel chunks per region, regions per band, regions
};

struct SaArgs {
    somi_slice x;
    somi_slice y;                                      // dout of the two backward passes
    somi_slice out;                                    // apply: out;  bwd input: dx
    float *stats, *sums, *part;                        // part: per-chunk partials (nP > 1)
    int add_input, accumulate;
    SaGeom g;
    SaPlan p;
};

static int sa_last_len(int size, int n, int step, int len, int stretch) { return stretch ? size - (n - 1) * step : len; }

static SaPlan sa_plan(int B, int H, int W, int C, int ny, int nx, int sy, int sx, int ly, int lx, int stretch) {
    SaPlan p;
    const MapShape s = map_shape(C);
    p.QW = s.QW; p.NL = s.NL; p.nQc = s.nQc;
    p.R = ny * nx;
    const long nmax = (long)sa_last_len(H, ny, sy, ly, stretch) * sa_last_len(W, nx, sx, lx, stretch);
    p.nP = cdiv(nmax, (long)SA_K * p.NL);
    p.RB = 8;
    while (p.RB > 1 && (long)B * p.nQc * p.nP * cdiv(p.R, p.RB) < 1024) p.RB /= 2;
    return p;
}

struct SaCover { int lo, n; };    // the regions lo .. lo + n - 1 of an axis cover a coordinate; n <= 0: none

__device__ __forceinline__ SaCover sa_cover(int p, int step, int len, int nreg, int stretch) {
    const int hi = min(nreg - 1, p / step);
    int lo = p >= len ? (p - len) / step + 1 : 0;
    if (stretch) lo = min(lo, nreg - 1);
    return SaCover{lo, hi - lo + 1};
}

struct SaRegion { int y0, x0, h, w; };

__device__ __forceinline__ SaRegion sa_region(const SaGeom &g, int r) {
    const int i = r / g.nx, j = r - i * g.nx;
    SaRegion q;
    q.y0 = i * g.sy;
    q.x0 = j * g.sx;
    q.h = (g.stretch && i == g.ny - 1) ? g.H - q.y0 : g.ly;
    q.w = (g.stretch && j == g.nx - 1) ? g.W - q.x0 : g.lx;
    return q;
}

// 1 / k of region (i, j) at pixel (h, w), which it covers
__device__ __forceinline__ float sa_weight(const SaGeom &g, int i, int j, int h, int w) {
    const SaCover cy = sa_cover(h, g.sy, g.ly, g.ny, g.stretch), cx = sa_cover(w, g.sx, g.lx, g.nx, g.stretch);
    return 1.0f / (float)((i - cy.lo) * cx.n + (j - cx.lo) + 1);
}

__device__ __forceinline__ f32x4 sa_sigmoid(f32x4 u) {
    f32x4 s;
    s.x = sigmoidf_(u.x); s.y = sigmoidf_(u.y); s.z = sigmoidf_(u.z); s.w = sigmoidf_(u.w);
    return s;
}

// (count, mean, M2) of two disjoint sets into the first; the counts depend on the lane or chunk only, never on the channel
__device__ __forceinline__ void sa_merge(float &na, f32x4 &ma, f32x4 &qa, float nb, const f32x4 &mb, const f32x4 &qb) {
    if (nb == 0.f) return;
    if (na == 0.f) { na = nb; ma = mb; qa = qb; return; }
    const float n = na + nb;
    const f32x4 delta = mb - ma;
    ma += delta * (nb / n);
    qa += qb + delta * delta * (na * nb / n);
    na = n;
}

// ------------------------------------------------------------------------------------------------ the two reductions, stage 1
// BWD = false: (mean, M2) of x per (region, chunk).  BWD = true: (A, B) of the backward.
template <bool BWD>
__global__ __launch_bounds__(256) void sa_reduce_kernel(SaArgs a) {
    __shared__ f32x4 s0[256], s1[256];
    __shared__ float scnt[256];
    const SaGeom &g = a.g;
    const int t = threadIdx.x, QW = a.p.QW, NL = a.p.NL, R = a.p.R;
    const int lane = t / QW, qq = t - lane * QW;
    const int b = blockIdx.z / a.p.nQc;
    const int q = (blockIdx.z - b * a.p.nQc) * 256 + qq;
    const bool on = lane < NL && q < g.C4;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    int top = 1;
    while (top < NL) top *= 2;
    const int r_end = min(R, ((int)blockIdx.y + 1) * a.p.RB);
    for (int r = blockIdx.y * a.p.RB; r < r_end; ++r) {
        const SaRegion rg = sa_region(g, r);
        const int ri = r / g.nx, rj = r - ri * g.nx;
        const int N = rg.h * rg.w;
        const int e0 = blockIdx.x * (SA_K * NL) + lane;
        f32x4 v[SA_K], dv[SA_K], mu = zero, dd = {1.f, 1.f, 1.f, 1.f};
        float wgt[SA_K], cnt = 0.f;
        if (BWD && on) {
            const float *st = a.stats + ((long)b * R + r) * 2 * (4 * g.C4) + 4 * q;
            mu = ld4(st);
            dd = 4.0f * (ld4(st + 4 * g.C4) * g.inv_n + g.lambda);
        }
#pragma unroll
        for (int k = 0; k < SA_K; ++k) {
            const int e = e0 + k * NL;
            v[k] = dv[k] = zero;
            wgt[k] = 0.f;
            if (on && e < N) {
                const int ey = e / rg.w, ex = e - ey * rg.w;
                const long pix = ((long)b * g.H + rg.y0 + ey) * g.W + rg.x0 + ex;
                v[k] = ld4(at(a.x, pix, q));
                if (BWD) {
                    dv[k] = ld4(at(a.y, pix, q));
                    wgt[k] = sa_weight(g, ri, rj, rg.y0 + ey, rg.x0 + ex);
                }
                cnt += 1.f;
            }
        }
        f32x4 m0 = zero, m1 = zero;                             // (mean, M2) or (A, B) of this lane
        if (BWD) {
#pragma unroll
            for (int k = 0; k < SA_K; ++k) {
                if ((float)k < cnt) {                            // a lane's pixels fill its slots from 0 up; small windows use few
                    const f32x4 d = v[k] - mu, d2 = d * d;
                    const f32x4 s = sa_sigmoid(d2 / dd + 0.5f);
                    const f32x4 T = wgt[k] * dv[k] * v[k] * s * (1.0f - s);
                    m0 += T * d;
                    m1 += T * d2;
                }
            }
        } else if (cnt > 0.f) {
#pragma unroll
            for (int k = 0; k < SA_K; ++k) m0 += v[k];          // the unused slots hold zeros
            m0 = m0 / cnt;
#pragma unroll
            for (int k = 0; k < SA_K; ++k) {
                const f32x4 d = v[k] - m0;
                if ((float)k < cnt) m1 += d * d;                 // a lane's pixels fill its slots from 0 up
            }
        }
        // lanes in a fixed tree: at width s lane l takes lane l + s
        s0[t] = m0; s1[t] = m1; scnt[t] = cnt;
        for (int s = top / 2; s >= 1; s /= 2) {
            __syncthreads();
            if (lane < s && lane + s < NL) {
                const int o = t + s * QW;
                if (BWD) {
                    m0 += s0[o];
                    m1 += s1[o];
                } else {
                    sa_merge(cnt, m0, m1, scnt[o], s0[o], s1[o]);
                    scnt[t] = cnt;
                }
                s0[t] = m0; s1[t] = m1;
            }
        }
        if (on && lane == 0) {
            float *dst = a.p.nP > 1 ? a.part + (((long)b * R + r) * a.p.nP + blockIdx.x) * 2 * (4 * g.C4)
                                    : (BWD ? a.sums : a.stats) + ((long)b * R + r) * 2 * (4 * g.C4);
            st4(dst + 4 * q, m0);
            st4(dst + 4 * g.C4 + 4 * q, m1);
        }
        __syncthreads();                                          // the next region reuses the LDS rows
    }
}

// stage 2 (nP > 1): one lane per (image, region, quad) merges its chunks in order
template <bool BWD>
__global__ __launch_bounds__(256) void sa_reduce_finish_kernel(SaArgs a, int B) {
    const SaGeom &g = a.g;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)B * a.p.R * g.C4) return;
    const int q = (int)(i % g.C4);
    const long br = i / g.C4;
    const int r = (int)(br % a.p.R);
    const SaRegion rg = sa_region(g, r);
    const int N = rg.h * rg.w, chunk = SA_K * a.p.NL;
    const float *src = a.part + br * a.p.nP * 2 * (4 * g.C4) + 4 * q;
    f32x4 m0 = {0.f, 0.f, 0.f, 0.f}, m1 = m0;
    float cnt = 0.f;
    for (int k = 0; k < a.p.nP; ++k, src += 2 * (4 * g.C4)) {
        const int have = min(chunk, N - k * chunk);
        if (have <= 0) break;                                     // a region smaller than the largest one has fewer chunks
        if (BWD) {
            m0 += ld4(src);
            m1 += ld4(src + 4 * g.C4);
        } else {
            sa_merge(cnt, m0, m1, (float)have, ld4(src), ld4(src + 4 * g.C4));
        }
    }
    float *dst = (BWD ? a.sums : a.stats) + br * 2 * (4 * g.C4) + 4 * q;
    st4(dst, m0);
    st4(dst + 4 * g.C4, m1);
}

// ------------------------------------------------------------------------------------------------ the two element-wise passes
// one lane per (pixel, quad); the statistics of the at most SA_COVER x SA_COVER regions over the pixel come from cache
template <bool BWD>
__global__ __launch_bounds__(256) void sa_apply_kernel(SaArgs a, long total) {
    const SaGeom &g = a.g;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int q = (int)(i % g.C4);
    const long pix = i / g.C4;
    const int w = (int)(pix % g.W);
    const long bh = pix / g.W;
    const int h = (int)(bh % g.H), b = (int)(bh / g.H);
    const int R = a.p.R;
    // x and o spelled out: through at() the forward instance schedules differently
    const f32x4 x = ld4(a.x.p + pix * a.x.cs + a.x.coff + 4 * q);
    f32x4 gr = {0.f, 0.f, 0.f, 0.f}, acc = gr;
    if (BWD) gr = ld4(at(a.y, pix, q));
    if (a.add_input) acc = BWD ? gr : x;
    const SaCover cy = sa_cover(h, g.sy, g.ly, g.ny, g.stretch), cx = sa_cover(w, g.sx, g.lx, g.nx, g.stretch);
    if (cy.n > 0 && cx.n > 0) {
        int k = 0;
        for (int i2 = cy.lo; i2 < cy.lo + cy.n; ++i2)
            for (int j2 = cx.lo; j2 < cx.lo + cx.n; ++j2) {
                const int r = i2 * g.nx + j2;
                const float wgt = 1.0f / (float)(++k);
                const float *st = a.stats + ((long)b * R + r) * 2 * (4 * g.C4) + 4 * q;
                const f32x4 d = x - ld4(st), d2 = d * d;
                const f32x4 dd = 4.0f * (ld4(st + 4 * g.C4) * g.inv_n + g.lambda);
                const f32x4 s = sa_sigmoid(d2 / dd + 0.5f);
                if (!BWD) {
                    acc += wgt * x * s;
                } else {
                    const SaRegion rg = sa_region(g, r);
                    const float *sm = a.sums + ((long)b * R + r) * 2 * (4 * g.C4) + 4 * q;
                    const f32x4 T = wgt * gr * x * s * (1.0f - s);
                    acc += wgt * gr * s + 2.0f * T * d / dd - ld4(sm) * (2.0f / (float)(rg.h * rg.w)) / dd
                           - (8.0f * g.inv_n) * d * ld4(sm + 4 * g.C4) / (dd * dd);
                }
            }
    }
    float *o = a.out.p + pix * a.out.cs + a.out.coff + 4 * q;
    if (BWD && a.accumulate) acc += ld4(o);
    st4(o, acc);
}

enum SaOp { SA_STATS, SA_APPLY, SA_SUMS_BWD, SA_INPUT_BWD };

// checks the descriptor for `op` and fills the kernel arguments; nothing is launched on an error
static int sa_unpack(const somi_simam_desc *d, SaOp op, SaArgs &a, const char *who) {
    SOMI_REQUIRE(d, SOMI_EINVAL, "%s: no descriptor", who);
    SOMI_REQUIRE(d->B > 0 && d->H > 0 && d->W > 0 && d->C > 0 && d->C % 4 == 0 && (long)d->B * d->H * d->W < (1L << 31) &&
                 (long)d->B * cdiv(d->C / 4, 256) <= 65535,
                 SOMI_EINVAL, "%s: bad sizes (C a multiple of 4, fewer than 2^31 pixels)", who);
    SOMI_REQUIRE(d->ny > 0 && d->nx > 0 && d->step_y > 0 && d->step_x > 0 && d->len_y > 0 && d->len_x > 0 &&
                 (long)(d->ny - 1) * d->step_y + d->len_y <= d->H && (long)(d->nx - 1) * d->step_x + d->len_x <= d->W &&
                 (long)d->ny * d->nx * d->B * (d->C / 4) < (1L << 31),
                 SOMI_EINVAL, "%s: bad region grid (ny x nx regions of len_y x len_x at steps step_y, step_x inside the H x W map)", who);
    SOMI_REQUIRE((long)d->len_y * d->len_x >= 2, SOMI_EINVAL, "%s: a region of one pixel has no variance (len_y * len_x >= 2)", who);
    SOMI_REQUIRE(cdiv(d->len_y, d->step_y) <= SA_COVER && cdiv(d->len_x, d->step_x) <= SA_COVER, SOMI_ENOTIMPL,
                 "%s: more than %d regions cover a pixel along one axis", who, SA_COVER);
    SOMI_REQUIRE(!d->stretch_last || (d->step_y == d->len_y && d->step_x == d->len_x), SOMI_EINVAL,
                 "%s: stretch_last needs regions that do not overlap (step == len)", who);
    SOMI_REQUIRE(d->n > 0.f && d->lambda > 0.f && d->n < 3e38f && d->lambda < 3e38f, SOMI_EINVAL,
                 "%s: the divisor n and lambda must be positive (lambda = 0 divides 0 by 0 on a constant channel, pad channels included)", who);
    const int C = d->C;
    SOMI_REQUIRE(d->stats && aligned16(d->stats), SOMI_EINVAL, "%s: stats (B, ny * nx, 2, C) must be given, 16-byte aligned", who);
    if (op == SA_SUMS_BWD || op == SA_INPUT_BWD)
        SOMI_REQUIRE(d->sums && aligned16(d->sums), SOMI_EINVAL, "%s: sums (B, ny * nx, 2, C) must be given, 16-byte aligned", who);
    if (op == SA_STATS) SOMI_REQUIRE_SLICES(who, {"x", d->x.p, d->x.cs, d->x.coff, C});
    if (op == SA_APPLY) SOMI_REQUIRE_SLICES(who, {"x", d->x.p, d->x.cs, d->x.coff, C}, {"out", d->y.p, d->y.cs, d->y.coff, C});
    if (op == SA_SUMS_BWD) SOMI_REQUIRE_SLICES(who, {"x", d->x.p, d->x.cs, d->x.coff, C}, {"dout", d->y.p, d->y.cs, d->y.coff, C});
    if (op == SA_INPUT_BWD)
        SOMI_REQUIRE_SLICES(who, {"x", d->x.p, d->x.cs, d->x.coff, C}, {"dout", d->y.p, d->y.cs, d->y.coff, C},
                            {"dx", d->dx.p, d->dx.cs, d->dx.coff, C});
    a = SaArgs{};
    a.p = sa_plan(d->B, d->H, d->W, C, d->ny, d->nx, d->step_y, d->step_x, d->len_y, d->len_x, d->stretch_last);
    SOMI_REQUIRE(cdiv(a.p.R, a.p.RB) <= 65535, SOMI_EINVAL, "%s: too many regions", who);
    if ((op == SA_STATS || op == SA_SUMS_BWD) && a.p.nP > 1) {
        SOMI_REQUIRE(d->workspace && aligned16(d->workspace), SOMI_EINVAL, "%s: a 16-byte aligned workspace is required", who);
        SOMI_REQUIRE(d->workspace_floats >= somi_simam_workspace_floats(d), SOMI_EWORKSPACE, "%s: workspace too small", who);
    }
    a.x = d->x; a.y = d->y;
    if (op == SA_APPLY) a.out = d->y;
    if (op == SA_INPUT_BWD) a.out = d->dx;
    a.stats = d->stats; a.sums = d->sums; a.part = d->workspace;
    a.add_input = d->add_input; a.accumulate = d->accumulate;
    a.g = SaGeom{d->H, d->W, C / 4, d->ny, d->nx, d->step_y, d->step_x, d->len_y, d->len_x, d->stretch_last ? 1 : 0, 1.0f / d->n, d->lambda};
    return 0;
}

template <bool BWD>
static void sa_reduce(const somi_simam_desc *d, const SaArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(sa_reduce_kernel<BWD>, dim3(a.p.nP, cdiv(a.p.R, a.p.RB), d->B * a.p.nQc), dim3(256), 0, s, a);
    if (a.p.nP > 1)
        hipLaunchKernelGGL(sa_reduce_finish_kernel<BWD>, dim3(cdiv((long)d->B * a.p.R * a.g.C4, 256)), dim3(256), 0, s, a, d->B);
}

template <bool BWD>
static void sa_apply(const somi_simam_desc *d, const SaArgs &a, hipStream_t s) {
    const long total = (long)d->B * d->H * d->W * a.g.C4;
    hipLaunchKernelGGL(sa_apply_kernel<BWD>, dim3(cdiv(total, 256)), dim3(256), 0, s, a, total);
}

}  // namespace somi

using namespace somi;

extern "C" size_t somi_simam_desc_bytes(void) { return sizeof(somi_simam_desc); }

extern "C" size_t somi_simam_workspace_floats(const somi_simam_desc *d) {
    if (!d || d->B <= 0 || d->H <= 0 || d->W <= 0 || d->C <= 0 || d->C % 4 || d->ny <= 0 || d->nx <= 0 || d->step_y <= 0 || d->step_x <= 0 ||
        d->len_y <= 0 || d->len_x <= 0 || (long)(d->ny - 1) * d->step_y + d->len_y > d->H || (long)(d->nx - 1) * d->step_x + d->len_x > d->W)
        return 0;
    const SaPlan p = sa_plan(d->B, d->H, d->W, d->C, d->ny, d->nx, d->step_y, d->step_x, d->len_y, d->len_x, d->stretch_last);
    return p.nP > 1 ? (size_t)d->B * p.R * p.nP * 2 * d->C : 0;
}

extern "C" int somi_simam_stats_nhwc_f32(const somi_simam_desc *d, somi_stream_t stream) {
    SaArgs a;
    if (int rc = sa_unpack(d, SA_STATS, a, "simam stats")) return rc;
    sa_reduce<false>(d, a, (hipStream_t)stream);
    return launch_status("somi_simam_stats_nhwc_f32");
}

extern "C" int somi_simam_apply_nhwc_f32(const somi_simam_desc *d, somi_stream_t stream) {
    SaArgs a;
    if (int rc = sa_unpack(d, SA_APPLY, a, "simam apply")) return rc;
    sa_apply<false>(d, a, (hipStream_t)stream);
    return launch_status("somi_simam_apply_nhwc_f32");
}

extern "C" int somi_simam_bwd_sums_nhwc_f32(const somi_simam_desc *d, somi_stream_t stream) {
    SaArgs a;
    if (int rc = sa_unpack(d, SA_SUMS_BWD, a, "simam bwd sums")) return rc;
    sa_reduce<true>(d, a, (hipStream_t)stream);
    return launch_status("somi_simam_bwd_sums_nhwc_f32");
}

extern "C" int somi_simam_bwd_input_nhwc_f32(const somi_simam_desc *d, somi_stream_t stream) {
    SaArgs a;
    if (int rc = sa_unpack(d, SA_INPUT_BWD, a, "simam bwd input")) return rc;
    sa_apply<true>(d, a, (hipStream_t)stream);
    return launch_status("somi_simam_bwd_input_nhwc_f32");
}
