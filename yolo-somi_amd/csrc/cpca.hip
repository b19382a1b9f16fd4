// Channel prior convolutional attention (CPCA / CPCABottleneck, models/common.py:5753-5859): the strip part
//   s = u + V7(H7(u)) + V11(H11(u)) + V21(H21(u)),   H_k the depthwise (1, k) conv along W, V_k the depthwise (k, 1) conv along H, all with bias,
// and the short element-wise passes around it.  The rest of the block (the 1x1 conv used three times, GELU, the depthwise 5x5, the global pools,
// the channel scale) runs on the entries that already exist.
//
//   fan-out  t_k = S_k(u) [+ b_k], k = 7, 11, 21: one tensor in, three out, u read once                       (4 tensor passes)
//   fan-in   s = [s +] p + sum_k (S_k(t_k) [+ b_k]): three tensors and the pass-through p in, one out         (5 tensor passes)
// each along W or along H and with the taps as stored or flipped: the forward is fan-out along W, fan-in along H; the data gradient is fan-out
// along H of ds with flipped taps (dt_k), then fan-in along W with flipped taps (du = ds + sum_k H_k^T dt_k).
//
// Geometry.  A lane owns a channel quad (adjacent lanes adjacent quads, at most 16 quads = 256 contiguous bytes per pixel and workgroup; wider
// tensors go over blockIdx.z) and CP_R = 4 consecutive outputs along the strip.  A workgroup's 256 lanes are QW quads x NA lanes along the strip
// x NO lines across it; it stages the (NA * 4 + 2 * halo) x NO pixels it reads in LDS (at most 1344 float4 = 21 KiB) beside the 39 tap vectors
// of its quads (at most 10 KiB) and walks LPW such tiles with the taps kept.  The tap loop is outermost in the lane: a tap vector is read from
// LDS once per tile and meets 4 window reads; a window address of lane (q, a) is (a * 4 + r + j) * QW + q float4, so the 16 lanes ds_read_b128
// serves per cycle read 256 contiguous bytes or runs of them 1 KiB apart - no bank conflict at QW = 16 (at QW = 8 two lanes 512 B apart share banks).  Twelve (fan-out) or four (fan-in)
// float4 accumulators per lane.  The tap loop stays rolled: unrolled, the compiler hoists all 39 tap vectors and the window into registers
// (256 VGPRs, one wave per SIMD); rolled it is 124 (fan-out, 4 waves per SIMD) and 80 (fan-in, 5), next to 31.5 KiB of LDS (5 workgroups per
// CU).  Along H the tile is [position][line][quad], along W [line][position][quad]: the global reads that fill it are contiguous along W.
//
// Weight and bias gradients (somi_cpca_wgrad_nhwc_f32): 78 tap sums and 4 distinct bias sums per channel.  Two stage-1 launches, one per axis,
// over tiles of at most 32 positions: lane (q, tl) owns up to three of the axis's 42 / 40 sums and keeps them in registers over its
// workgroup's tiles; the four tensors of a step (one halo tile and three gradient tiles along W, three halo tiles and one gradient tile along
// H, 37 / 47 KiB) are in LDS together, so every lane works at once (the gradient read is a broadcast among the lanes of a quad); each
// workgroup leaves one row of partials.  Stage 2: 16 lanes per (sum, channel) add the rows in a fixed interleave and a fixed LDS tree.
// No float atomics anywhere: two launches are bit-identical.
#include "common.h"

namespace somi {

constexpr int CP_R = 4;                   // outputs per lane along the strip
constexpr int CP_HALO = 10;               // 21 / 2
constexpr int CP_TAMAX = 64;              // strip positions of a tile
constexpr int CP_QWMAX = 16;              // quads of a workgroup
constexpr int CP_TILE = (CP_TAMAX + 2 * CP_HALO) * CP_QWMAX;
constexpr int CP_WG_TAMAX = 32;           // the weight-gradient kernel holds four tiles at once: shorter ones
constexpr int CP_WG_TILE = (CP_WG_TAMAX + 2 * CP_HALO) * CP_QWMAX, CP_WG_DTILE = CP_WG_TAMAX * CP_QWMAX;
constexpr int CP_NTAP = 39;               // 7 + 11 + 21
constexpr int CP_NTASK_W = 42, CP_NTASK_H = 40;

__host__ __device__ constexpr int cp_taps(int k) { return k == 0 ? 7 : (k == 1 ? 11 : 21); }
__host__ __device__ constexpr int cp_base(int k) { return k == 0 ? 0 : (k == 1 ? 7 : 18); }

struct CpPlan { int QW, nQc, NA, NO, TA, nA, LPW, nO, LA, LO, SA, SO; };

// axis 0: strips along W, 1: along H.  lpw0 / fill: the workgroup walks up to lpw0 tiles, halved until `fill` workgroups exist
static CpPlan cp_plan(int B, int H, int W, int C, int axis, int lpw0, int fill, int tamax = CP_TAMAX) {
    CpPlan p;
    const int C4 = C / 4;
    p.LA = axis ? H : W; p.LO = axis ? W : H;
    p.SA = axis ? W : 1; p.SO = axis ? 1 : W;
    p.QW = C4 < CP_QWMAX ? C4 : CP_QWMAX;
    p.nQc = cdiv(C4, CP_QWMAX);
    const int NL = 256 / p.QW;
    p.NA = cdiv(p.LA, CP_R) < tamax / CP_R ? cdiv(p.LA, CP_R) : tamax / CP_R;
    p.TA = p.NA * CP_R;
    p.NO = NL / p.NA;
    const int fit = (tamax + 2 * CP_HALO) * CP_QWMAX / ((p.TA + 2 * CP_HALO) * p.QW);
    if (p.NO > fit) p.NO = fit;
    if (p.NO > p.LO) p.NO = p.LO;
    p.nA = cdiv(p.LA, p.TA);
    p.LPW = lpw0;
    while (p.LPW > 1 && (long)B * p.nQc * p.nA * cdiv(p.LO, p.NO * p.LPW) < fill) p.LPW /= 2;
    p.nO = cdiv(p.LO, p.NO * p.LPW);
    return p;
}

struct CpGeom { int H, W, C4, SA, SO, LA, LO, QW, nQc, NA, NO, TA, LPW, alongw; };

static CpGeom cp_geom(int H, int W, int C, const CpPlan &p) {
    return CpGeom{H, W, C / 4, p.SA, p.SO, p.LA, p.LO, p.QW, p.nQc, p.NA, p.NO, p.TA, p.LPW, p.SA == 1};
}

struct CpArgs {
    somi_slice src[4], dst[3];
    const float *w[3], *bias[3];
    int flip, accumulate;
    CpGeom g;
};

// the tile of `s` around strip positions [a0 - halo, a0 + TA + halo) of lines [o0, o0 + NO), zero outside the map: [line][position][quad] along W,
// [position][line][quad] along H
__device__ __forceinline__ void cp_load_tile(f32x4 *tile, const somi_slice &s, const CpGeom &g, long img, int qc, int a0, int o0, int halo) {
    const int TI = g.TA + 2 * halo, n = TI * g.NO * g.QW;
    for (int idx = threadIdx.x; idx < n; idx += 256) {
        const int qq = idx % g.QW, rest = idx / g.QW;
        const int i = g.alongw ? rest % TI : rest / g.NO, o = g.alongw ? rest / TI : rest % g.NO;
        const int pa = a0 - halo + i, po = o0 + o, qg = qc * CP_QWMAX + qq;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (qg < g.C4 && pa >= 0 && pa < g.LA && po < g.LO)
            v = ld4(at(s, img + (long)pa * g.SA + (long)po * g.SO, qg));
        tile[idx] = v;
    }
}

// tile index of (position i of the tile, line o, quad q)
__device__ __forceinline__ int cp_at(const CpGeom &g, int TI, int i, int o, int q) {
    return ((g.alongw ? o * TI + i : i * g.NO + o)) * g.QW + q;
}

__device__ __forceinline__ f32x4 cp_chan4(const float *p, int c, int stride) {
    return f32x4{p[(long)c * stride], p[(long)(c + 1) * stride], p[(long)(c + 2) * stride], p[(long)(c + 3) * stride]};
}

// the 39 tap vectors of the workgroup's quads, [tap][quad]; weights are (C, k) as nn.Conv2d stores (C,1,1,k) and (C,1,k,1); no alignment assumed
__device__ __forceinline__ void cp_load_taps(f32x4 *sw, const float *w0, const float *w1, const float *w2, int flip, const CpGeom &g, int qc) {
    for (int i = threadIdx.x; i < CP_NTAP * g.QW; i += 256) {
        const int qq = i % g.QW, tp = i / g.QW;
        const int k = tp < 7 ? 0 : (tp < 18 ? 1 : 2), K = cp_taps(k);
        int tap = tp - cp_base(k);
        if (flip) tap = K - 1 - tap;
        const float *w = k == 0 ? w0 : (k == 1 ? w1 : w2);
        const int qg = qc * CP_QWMAX + qq;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (qg < g.C4) v = cp_chan4(w + tap, 4 * qg, K);
        sw[i] = v;
    }
}

template <bool FANIN>
__global__ __launch_bounds__(256) void cp_strip_kernel(CpArgs a) {
    __shared__ f32x4 tile[CP_TILE];
    __shared__ f32x4 sw[CP_NTAP * CP_QWMAX];
    const CpGeom &g = a.g;
    const int t = threadIdx.x;
    const int q = t % g.QW, l = t / g.QW;
    const int la = l % g.NA, lo = l / g.NA;
    const int b = blockIdx.z / g.nQc, qc = blockIdx.z - b * g.nQc;
    const int qg = qc * CP_QWMAX + q;
    const bool on = qg < g.C4 && lo < g.NO;
    const long img = (long)b * g.H * g.W;
    const int a0 = blockIdx.x * g.TA;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    cp_load_taps(sw, a.w[0], a.w[1], a.w[2], a.flip, g, qc);
    f32x4 bs[3] = {zero, zero, zero};
    if (on) {
        if (a.bias[0]) bs[0] = cp_chan4(a.bias[0], 4 * qg, 1);
        if (a.bias[1]) bs[1] = cp_chan4(a.bias[1], 4 * qg, 1);
        if (a.bias[2]) bs[2] = cp_chan4(a.bias[2], 4 * qg, 1);
    }
    for (int it = 0; it < g.LPW; ++it) {
        const int o0 = (blockIdx.y * g.LPW + it) * g.NO;
        if (o0 >= g.LO) break;
        const int po = o0 + lo, pa0 = a0 + la * CP_R;
        const bool lane = on && po < g.LO;
        const long pix0 = img + (long)pa0 * g.SA + (long)po * g.SO;
        if (!FANIN) {
            __syncthreads();
            cp_load_tile(tile, a.src[0], g, img, qc, a0, o0, CP_HALO);
            __syncthreads();
            if (!lane) continue;
            const int TI = g.TA + 2 * CP_HALO;
            f32x4 acc[3][CP_R];
#pragma unroll
            for (int r = 0; r < CP_R; ++r) acc[0][r] = acc[1][r] = acc[2][r] = zero;
#pragma unroll 1
            for (int j = 0; j <= 2 * CP_HALO; ++j) {              // rolled: unrolled, the compiler keeps every tap and the window in registers
                const f32x4 w21 = sw[(18 + j) * g.QW + q];
                f32x4 w11 = zero, w7 = zero;
                if (j >= 5 && j <= 15) w11 = sw[(7 + j - 5) * g.QW + q];
                if (j >= 7 && j <= 13) w7 = sw[(j - 7) * g.QW + q];
#pragma unroll
                for (int r = 0; r < CP_R; ++r) {
                    const f32x4 v = tile[cp_at(g, TI, la * CP_R + r + j, lo, q)];
                    acc[2][r] += w21 * v;
                    if (j >= 5 && j <= 15) acc[1][r] += w11 * v;
                    if (j >= 7 && j <= 13) acc[0][r] += w7 * v;
                }
            }
#pragma unroll
            for (int r = 0; r < CP_R; ++r) {
                if (pa0 + r >= g.LA) break;
                const long pix = pix0 + (long)r * g.SA;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const f32x4 o = acc[k][r] + bs[k];
                    st4(at_w(a.dst[k], pix, qg), o);
                }
            }
        } else {
            f32x4 acc[CP_R];
#pragma unroll
            for (int r = 0; r < CP_R; ++r) {
                acc[r] = zero;
                if (lane && pa0 + r < g.LA) {
                    const long pix = pix0 + (long)r * g.SA;
                    acc[r] = ld4(at(a.src[3], pix, qg)) + (bs[0] + bs[1] + bs[2]);
                    if (a.accumulate) acc[r] += ld4(at(a.dst[0], pix, qg));
                }
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int halo = cp_taps(k) / 2, TI = g.TA + 2 * halo;
                __syncthreads();
                cp_load_tile(tile, a.src[k], g, img, qc, a0, o0, halo);
                __syncthreads();
                if (lane) {
#pragma unroll 1
                    for (int j = 0; j < cp_taps(k); ++j) {
                        const f32x4 w = sw[(cp_base(k) + j) * g.QW + q];
#pragma unroll
                        for (int r = 0; r < CP_R; ++r) acc[r] += w * tile[cp_at(g, TI, la * CP_R + r + j, lo, q)];
                    }
                }
            }
            if (!lane) continue;
#pragma unroll
            for (int r = 0; r < CP_R; ++r) {
                if (pa0 + r >= g.LA) break;
                const long pix = pix0 + (long)r * g.SA;
                st4(at_w(a.dst[0], pix, qg), acc[r]);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ weight and bias gradients
struct CpWArgs {
    somi_slice A[3], D[3];            // along W: A[0] = u read with a halo, D[k] = dt_k;  along H: A[k] = t_k with a halo, D[0] = ds
    int ntask;
    float *part;                      // [rows][ntask][C]
    int nA, nO;
    CpGeom g;
};

// ALONGH = false: 42 sums - 7 taps, sum dt_7, 11 taps, sum dt_11, 21 taps, sum dt_21.  ALONGH = true: 40 sums - 7, 11, 21 taps, sum ds.
// All tiles of a step are in LDS at once, so every lane works on its sums at the same time: lane (q, tl) owns the sums tl, tl + NT, tl + 2 NT.
template <bool ALONGH>
__global__ __launch_bounds__(256) void cp_wgrad_kernel(CpWArgs a) {
    constexpr int NAT = ALONGH ? 3 : 1, NDT = ALONGH ? 1 : 3;
    __shared__ f32x4 tA[NAT][CP_WG_TILE];
    __shared__ f32x4 tD[NDT][CP_WG_DTILE];
    const CpGeom &g = a.g;
    const int t = threadIdx.x;
    const int q = t % g.QW, tl = t / g.QW, NT = 256 / g.QW;
    const int b = blockIdx.z / g.nQc, qc = blockIdx.z - b * g.nQc;
    const int qg = qc * CP_QWMAX + q;
    const bool on = qg < g.C4 && tl < NT;
    const long img = (long)b * g.H * g.W;
    const int a0 = blockIdx.x * g.TA;
    const int TI = g.TA + 2 * CP_HALO;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    // what each of the lane's three sums is: tap set k, offset into the halo tile (or -1: the plain sum of D)
    int kk[3], off[3];
#pragma unroll
    for (int rd = 0; rd < 3; ++rd) {
        const int task = tl + rd * NT;
        kk[rd] = 0; off[rd] = -2;                                 // -2: no sum
        if (!on || task >= a.ntask) continue;
        if (ALONGH) {
            if (task == CP_NTAP) { kk[rd] = 0; off[rd] = -1; continue; }
            const int k = task < 7 ? 0 : (task < 18 ? 1 : 2);
            kk[rd] = k; off[rd] = task - cp_base(k) + CP_HALO - cp_taps(k) / 2;
        } else {
            const int k = task < 8 ? 0 : (task < 20 ? 1 : 2), tap = task - (k == 0 ? 0 : (k == 1 ? 8 : 20));
            kk[rd] = k; off[rd] = tap < cp_taps(k) ? tap + CP_HALO - cp_taps(k) / 2 : -1;
        }
    }
    f32x4 acc[3] = {zero, zero, zero};
    for (int it = 0; it < g.LPW; ++it) {
        const int o0 = (blockIdx.y * g.LPW + it) * g.NO;
        if (o0 >= g.LO) break;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < NAT; ++k) cp_load_tile(tA[k], a.A[k], g, img, qc, a0, o0, CP_HALO);
#pragma unroll
        for (int k = 0; k < NDT; ++k) cp_load_tile(tD[k], a.D[k], g, img, qc, a0, o0, 0);
        __syncthreads();
#pragma unroll
        for (int rd = 0; rd < 3; ++rd) {
            if (off[rd] < -1) continue;
            const f32x4 *pd = tD[ALONGH ? 0 : kk[rd]], *pa = tA[ALONGH ? kk[rd] : 0];
            f32x4 s0 = zero, s1 = zero;
            for (int o = 0; o < g.NO; ++o) {
                if (off[rd] >= 0) {
#pragma unroll 4
                    for (int i = 0; i < g.TA; i += 2) {           // TA is a multiple of 4
                        s0 += pd[cp_at(g, g.TA, i, o, q)] * pa[cp_at(g, TI, i + off[rd], o, q)];
                        s1 += pd[cp_at(g, g.TA, i + 1, o, q)] * pa[cp_at(g, TI, i + 1 + off[rd], o, q)];
                    }
                } else {
#pragma unroll 4
                    for (int i = 0; i < g.TA; i += 2) {
                        s0 += pd[cp_at(g, g.TA, i, o, q)];
                        s1 += pd[cp_at(g, g.TA, i + 1, o, q)];
                    }
                }
            }
            acc[rd] += s0 + s1;
        }
    }
    const long row = ((long)b * a.nO + blockIdx.y) * a.nA + blockIdx.x;
#pragma unroll
    for (int rd = 0; rd < 3; ++rd) {
        const int task = tl + rd * NT;
        if (on && task < a.ntask) st4(a.part + (row * a.ntask + task) * (4L * g.C4) + 4 * qg, acc[rd]);
    }
}

struct CpFoldArgs {
    const float *part_w, *part_h;
    long rows_w, rows_h;
    float *dw_h[3], *dw_v[3], *db_h[3], *db_v[3];
    int accumulate, C;
};

// one workgroup per (sum, 16 channels): 16 lanes per sum take the rows 16 apart in order, then a fixed tree
__global__ __launch_bounds__(256) void cp_wgrad_fold_kernel(CpFoldArgs a) {
    __shared__ float sh[256];
    const int t = threadIdx.x, cx = t % 16, rl = t / 16;
    const int c = blockIdx.x * 16 + cx;
    const bool along_h = (int)blockIdx.y >= CP_NTASK_W;
    const int task = along_h ? blockIdx.y - CP_NTASK_W : blockIdx.y, ntask = along_h ? CP_NTASK_H : CP_NTASK_W;
    const float *part = along_h ? a.part_h : a.part_w;
    const long rows = along_h ? a.rows_h : a.rows_w;
    float s = 0.f;
    if (c < a.C)
        for (long r = rl; r < rows; r += 16) s += part[(r * ntask + task) * a.C + c];
    sh[t] = s;
    __syncthreads();
    for (int st = 8; st >= 1; st >>= 1) {
        if (rl < st) sh[t] += sh[t + st * 16];
        __syncthreads();
    }
    if (rl != 0 || c >= a.C) return;
    s = sh[t];
    float *dst[3] = {nullptr, nullptr, nullptr};
    if (!along_h) {                                   // 7 taps, bias, 11 taps, bias, 21 taps, bias
        const int k = task < 8 ? 0 : (task < 20 ? 1 : 2), tap = task - (k == 0 ? 0 : (k == 1 ? 8 : 20)), K = cp_taps(k);
        float *w = k == 0 ? a.dw_h[0] : (k == 1 ? a.dw_h[1] : a.dw_h[2]), *bb = k == 0 ? a.db_h[0] : (k == 1 ? a.db_h[1] : a.db_h[2]);
        dst[0] = tap < K ? (w ? w + (long)c * K + tap : nullptr) : (bb ? bb + c : nullptr);
    } else if (task < CP_NTAP) {                      // 7, 11, 21 taps
        const int k = task < 7 ? 0 : (task < 18 ? 1 : 2), tap = task - cp_base(k), K = cp_taps(k);
        float *w = k == 0 ? a.dw_v[0] : (k == 1 ? a.dw_v[1] : a.dw_v[2]);
        dst[0] = w ? w + (long)c * K + tap : nullptr;
    } else {                                          // the column sum of ds: the bias gradient of all three
        for (int k = 0; k < 3; ++k) dst[k] = a.db_v[k] ? a.db_v[k] + c : nullptr;
    }
    for (int k = 0; k < 3; ++k)
        if (dst[k]) *dst[k] = a.accumulate ? *dst[k] + s : s;
}

// ------------------------------------------------------------------------------------------------ the element-wise passes
// out = x * y;  backward: dx = dout * y, dy = dout * x
__global__ __launch_bounds__(256) void cp_gate_kernel(somi_slice x, somi_slice y, somi_slice out, long n4, int C4) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const long pix = i / C4;
    const int c = 4 * (int)(i - pix * C4);
    const f32x4 o = ld4(at_ch(x, pix, c)) * ld4(at_ch(y, pix, c));
    st4(at_ch_w(out, pix, c), o);
}

__global__ __launch_bounds__(256) void cp_gate_bwd_kernel(somi_slice dout, somi_slice x, somi_slice y, somi_slice dx, somi_slice dy, long n4, int C4) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const long pix = i / C4;
    const int c = 4 * (int)(i - pix * C4);
    const f32x4 d = ld4(at_ch(dout, pix, c));
    const f32x4 xv = ld4(at_ch(x, pix, c));
    const f32x4 yv = ld4(at_ch(y, pix, c));
    st4(at_ch_w(dx, pix, c), d * yv);
    st4(at_ch_w(dy, pix, c), d * xv);
}

// g[b][c] = sigmoid(z[b][c]) + sigmoid(z[B + b][c]);  backward: dz[b] = dg s1 (1 - s1), dz[B + b] = dg s2 (1 - s2)
__global__ __launch_bounds__(256) void cp_sigmoid2_kernel(const float *z, const float *dg, float *out, long n, int bwd) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float s1 = sigmoidf_(z[i]), s2 = sigmoidf_(z[n + i]);
    if (!bwd) {
        out[i] = s1 + s2;
    } else {
        out[i] = dg[i] * s1 * (1.f - s1);
        out[n + i] = dg[i] * s2 * (1.f - s2);
    }
}

constexpr int CP_AM_CHUNK = 64;
// amaxp[b][c] = the first pixel p with x[b,p,c] == mx[b][c] (an integer minimum over the matching pixels: independent of the order)
__global__ __launch_bounds__(256) void cp_argmax_kernel(somi_slice x, const float *mx, int *amaxp, int HW, int C) {
    const int c = blockIdx.y * 256 + threadIdx.x, b = blockIdx.z;
    if (c >= C) return;
    const int p0 = blockIdx.x * CP_AM_CHUNK, p1 = min(HW, p0 + CP_AM_CHUNK);
    const float m = mx[(long)b * C + c];
    for (int p = p0; p < p1; ++p)
        if (x.p[((long)b * HW + p) * x.cs + x.coff + c] == m) {
            atomicMin(amaxp + (long)b * C + c, p);
            return;
        }
}

static int cp_sizes_ok(int B, int H, int W, int C) {
    return B > 0 && H > 0 && W > 0 && C > 0 && (long)B * H * W < (1L << 31) && (long)B * cdiv(C / 4 > 0 ? C / 4 : 1, CP_QWMAX) <= 65535;
}

static int cp_strip_launch(const somi_cpca_strip_desc *d, bool fanin, somi_stream_t stream, const char *who) {
    SOMI_REQUIRE(d, SOMI_EINVAL, "%s: no descriptor", who);
    SOMI_REQUIRE(d->C > 0 && d->C % 4 == 0, SOMI_EINVAL, "%s: C = %d is not a multiple of 4 (a lane owns a channel quad)", who, d->C);
    SOMI_REQUIRE(d->taps[0] == 7 && d->taps[1] == 11 && d->taps[2] == 21, SOMI_EINVAL, "%s: tap set (%d, %d, %d) is not built, only (7, 11, 21)", who,
                 d->taps[0], d->taps[1], d->taps[2]);
    SOMI_REQUIRE(cp_sizes_ok(d->B, d->H, d->W, d->C), SOMI_EINVAL, "%s: bad sizes (fewer than 2^31 pixels)", who);
    SOMI_REQUIRE(d->axis == 0 || d->axis == 1, SOMI_EINVAL, "%s: axis is 0 (along W) or 1 (along H)", who);
    SOMI_REQUIRE(d->w[0] && d->w[1] && d->w[2], SOMI_EINVAL, "%s: three tap tensors are required", who);
    const int C = d->C;
    if (!fanin)
        SOMI_REQUIRE_SLICES(who, {"src[0]", d->src[0].p, d->src[0].cs, d->src[0].coff, C}, {"dst[0]", d->dst[0].p, d->dst[0].cs, d->dst[0].coff, C},
                            {"dst[1]", d->dst[1].p, d->dst[1].cs, d->dst[1].coff, C}, {"dst[2]", d->dst[2].p, d->dst[2].cs, d->dst[2].coff, C});
    else
        SOMI_REQUIRE_SLICES(who, {"src[0]", d->src[0].p, d->src[0].cs, d->src[0].coff, C}, {"src[1]", d->src[1].p, d->src[1].cs, d->src[1].coff, C},
                            {"src[2]", d->src[2].p, d->src[2].cs, d->src[2].coff, C}, {"src[3]", d->src[3].p, d->src[3].cs, d->src[3].coff, C},
                            {"dst[0]", d->dst[0].p, d->dst[0].cs, d->dst[0].coff, C});
    const CpPlan p = cp_plan(d->B, d->H, d->W, C, d->axis, 4, 1024);
    SOMI_REQUIRE(p.nO <= 65535, SOMI_EINVAL, "%s: map too large across the strip", who);
    CpArgs a;
    for (int i = 0; i < 4; ++i) a.src[i] = d->src[i];
    for (int i = 0; i < 3; ++i) { a.dst[i] = d->dst[i]; a.w[i] = d->w[i]; a.bias[i] = d->bias[i]; }
    a.flip = d->flip; a.accumulate = d->accumulate;
    a.g = cp_geom(d->H, d->W, C, p);
    const dim3 grid(p.nA, p.nO, d->B * p.nQc);
    if (fanin) hipLaunchKernelGGL(cp_strip_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(cp_strip_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, a);
    return launch_status(who);
}

static long cp_wgrad_rows(int B, int H, int W, int C, int axis, CpPlan *out = nullptr) {
    const CpPlan p = cp_plan(B, H, W, C, axis, 32, 512, CP_WG_TAMAX);
    if (out) *out = p;
    return (long)B * p.nO * p.nA;
}

}  // namespace somi

using namespace somi;

extern "C" size_t somi_cpca_strip_desc_bytes(void) { return sizeof(somi_cpca_strip_desc); }
extern "C" size_t somi_cpca_wgrad_desc_bytes(void) { return sizeof(somi_cpca_wgrad_desc); }

extern "C" int somi_cpca_fanout_nhwc_f32(const somi_cpca_strip_desc *d, somi_stream_t stream) {
    return cp_strip_launch(d, false, stream, "cpca fanout");
}

extern "C" int somi_cpca_fanin_nhwc_f32(const somi_cpca_strip_desc *d, somi_stream_t stream) {
    return cp_strip_launch(d, true, stream, "cpca fanin");
}

extern "C" int somi_cpca_tiles_per_workgroup(int B, int H, int W, int C, int axis, int wgrad) {
    if (C <= 0 || C % 4 || !cp_sizes_ok(B, H, W, C) || (axis != 0 && axis != 1)) return 0;
    return (wgrad ? cp_plan(B, H, W, C, axis, 32, 512, CP_WG_TAMAX) : cp_plan(B, H, W, C, axis, 4, 1024)).LPW;
}

extern "C" size_t somi_cpca_wgrad_workspace_floats(int B, int H, int W, int C) {
    if (C <= 0 || C % 4 || !cp_sizes_ok(B, H, W, C)) return 0;
    return (size_t)(cp_wgrad_rows(B, H, W, C, 0) * CP_NTASK_W + cp_wgrad_rows(B, H, W, C, 1) * CP_NTASK_H) * C;
}

extern "C" int somi_cpca_wgrad_nhwc_f32(const somi_cpca_wgrad_desc *d, somi_stream_t stream) {
    const char *who = "cpca wgrad";
    SOMI_REQUIRE(d, SOMI_EINVAL, "%s: no descriptor", who);
    SOMI_REQUIRE(d->C > 0 && d->C % 4 == 0, SOMI_EINVAL, "%s: C = %d is not a multiple of 4 (a lane owns a channel quad)", who, d->C);
    SOMI_REQUIRE(d->taps[0] == 7 && d->taps[1] == 11 && d->taps[2] == 21, SOMI_EINVAL, "%s: tap set (%d, %d, %d) is not built, only (7, 11, 21)", who,
                 d->taps[0], d->taps[1], d->taps[2]);
    SOMI_REQUIRE(cp_sizes_ok(d->B, d->H, d->W, d->C), SOMI_EINVAL, "%s: bad sizes (fewer than 2^31 pixels)", who);
    const int C = d->C;
    SOMI_REQUIRE_SLICES(who, {"u", d->u.p, d->u.cs, d->u.coff, C}, {"ds", d->ds.p, d->ds.cs, d->ds.coff, C},
                        {"t[0]", d->t[0].p, d->t[0].cs, d->t[0].coff, C}, {"t[1]", d->t[1].p, d->t[1].cs, d->t[1].coff, C},
                        {"t[2]", d->t[2].p, d->t[2].cs, d->t[2].coff, C}, {"dt[0]", d->dt[0].p, d->dt[0].cs, d->dt[0].coff, C},
                        {"dt[1]", d->dt[1].p, d->dt[1].cs, d->dt[1].coff, C}, {"dt[2]", d->dt[2].p, d->dt[2].cs, d->dt[2].coff, C});
    SOMI_REQUIRE(d->workspace && aligned16(d->workspace), SOMI_EINVAL, "%s: a 16-byte aligned workspace is required", who);
    SOMI_REQUIRE(d->workspace_floats >= somi_cpca_wgrad_workspace_floats(d->B, d->H, d->W, C), SOMI_EWORKSPACE, "%s: workspace too small", who);
    CpPlan pw, ph;
    const long rows_w = cp_wgrad_rows(d->B, d->H, d->W, C, 0, &pw), rows_h = cp_wgrad_rows(d->B, d->H, d->W, C, 1, &ph);
    SOMI_REQUIRE(pw.nO <= 65535 && ph.nO <= 65535, SOMI_EINVAL, "%s: map too large", who);
    float *part_w = d->workspace, *part_h = d->workspace + (size_t)rows_w * CP_NTASK_W * C;
    CpWArgs a;
    for (int k = 0; k < 3; ++k) { a.A[k] = d->u; a.D[k] = d->dt[k]; }
    a.ntask = CP_NTASK_W; a.part = part_w; a.nA = pw.nA; a.nO = pw.nO;
    a.g = cp_geom(d->H, d->W, C, pw);
    hipLaunchKernelGGL(cp_wgrad_kernel<false>, dim3(pw.nA, pw.nO, d->B * pw.nQc), dim3(256), 0, (hipStream_t)stream, a);
    for (int k = 0; k < 3; ++k) { a.A[k] = d->t[k]; a.D[k] = d->ds; }
    a.ntask = CP_NTASK_H; a.part = part_h; a.nA = ph.nA; a.nO = ph.nO;
    a.g = cp_geom(d->H, d->W, C, ph);
    hipLaunchKernelGGL(cp_wgrad_kernel<true>, dim3(ph.nA, ph.nO, d->B * ph.nQc), dim3(256), 0, (hipStream_t)stream, a);
    CpFoldArgs f;
    f.part_w = part_w; f.part_h = part_h; f.rows_w = rows_w; f.rows_h = rows_h;
    for (int k = 0; k < 3; ++k) { f.dw_h[k] = d->dw_h[k]; f.dw_v[k] = d->dw_v[k]; f.db_h[k] = d->db_h[k]; f.db_v[k] = d->db_v[k]; }
    f.accumulate = d->accumulate; f.C = C;
    hipLaunchKernelGGL(cp_wgrad_fold_kernel, dim3(cdiv(C, 16), CP_NTASK_W + CP_NTASK_H), dim3(256), 0, (hipStream_t)stream, f);
    return launch_status("somi_cpca_wgrad_nhwc_f32");
}

static int cp_pointwise_ok(const char *who, long npix, int C) {
    SOMI_REQUIRE(npix > 0 && npix < (1L << 31), SOMI_EINVAL, "%s: bad pixel count", who);
    SOMI_REQUIRE(C > 0 && C % 4 == 0, SOMI_EINVAL, "%s: C = %d is not a multiple of 4", who, C);
    return 0;
}

extern "C" int somi_cpca_gate_nhwc_f32(somi_slice x, somi_slice y, somi_slice out, long npix, int C, somi_stream_t stream) {
    const char *who = "cpca gate";
    if (int rc = cp_pointwise_ok(who, npix, C)) return rc;
    SOMI_REQUIRE_SLICES(who, {"x", x.p, x.cs, x.coff, C}, {"y", y.p, y.cs, y.coff, C}, {"out", out.p, out.cs, out.coff, C});
    const long n4 = npix * (C / 4);
    hipLaunchKernelGGL(cp_gate_kernel, dim3(cdiv(n4, 256)), dim3(256), 0, (hipStream_t)stream, x, y, out, n4, C / 4);
    return launch_status("somi_cpca_gate_nhwc_f32");
}

extern "C" int somi_cpca_gate_bwd_nhwc_f32(somi_slice dout, somi_slice x, somi_slice y, somi_slice dx, somi_slice dy, long npix, int C,
                                           somi_stream_t stream) {
    const char *who = "cpca gate bwd";
    if (int rc = cp_pointwise_ok(who, npix, C)) return rc;
    SOMI_REQUIRE_SLICES(who, {"dout", dout.p, dout.cs, dout.coff, C}, {"x", x.p, x.cs, x.coff, C}, {"y", y.p, y.cs, y.coff, C},
                        {"dx", dx.p, dx.cs, dx.coff, C}, {"dy", dy.p, dy.cs, dy.coff, C});
    const long n4 = npix * (C / 4);
    hipLaunchKernelGGL(cp_gate_bwd_kernel, dim3(cdiv(n4, 256)), dim3(256), 0, (hipStream_t)stream, dout, x, y, dx, dy, n4, C / 4);
    return launch_status("somi_cpca_gate_bwd_nhwc_f32");
}

extern "C" int somi_cpca_sigmoid2_f32(const float *z, float *g, int B, int C, somi_stream_t stream) {
    SOMI_REQUIRE(z && g && B > 0 && C > 0, SOMI_EINVAL, "cpca sigmoid2: bad arguments");
    const long n = (long)B * C;
    hipLaunchKernelGGL(cp_sigmoid2_kernel, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, z, (const float *)nullptr, g, n, 0);
    return launch_status("somi_cpca_sigmoid2_f32");
}

extern "C" int somi_cpca_sigmoid2_bwd_f32(const float *z, const float *dg, float *dz, int B, int C, somi_stream_t stream) {
    SOMI_REQUIRE(z && dg && dz && B > 0 && C > 0, SOMI_EINVAL, "cpca sigmoid2 bwd: bad arguments");
    const long n = (long)B * C;
    hipLaunchKernelGGL(cp_sigmoid2_kernel, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, z, dg, dz, n, 1);
    return launch_status("somi_cpca_sigmoid2_bwd_f32");
}

extern "C" int somi_cpca_argmax_pixel_nhwc_f32(somi_slice x, const float *mx, int32_t *amaxp, int B, int HW, int C, somi_stream_t stream) {
    const char *who = "cpca argmax pixel";
    SOMI_REQUIRE(mx && amaxp && B > 0 && B <= 65535 && HW > 0 && (long)B * HW < (1L << 31), SOMI_EINVAL, "%s: bad arguments", who);
    SOMI_REQUIRE_SLICES(who, {"x", x.p, x.cs, x.coff, C});
    if (hipMemsetAsync(amaxp, 0x7f, sizeof(int32_t) * (size_t)B * C, (hipStream_t)stream) != hipSuccess) return launch_status(who);
    hipLaunchKernelGGL(cp_argmax_kernel, dim3(cdiv(HW, CP_AM_CHUNK), cdiv(C, 256), B), dim3(256), 0, (hipStream_t)stream, x, mx, amaxp, HW, C);
    return launch_status("somi_cpca_argmax_pixel_nhwc_f32");
}
