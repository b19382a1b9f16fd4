// Swin window attention (SwinTransformerLayer / WindowAttention, models/common.py:1184-1358, inside C3STR :1632-1637), the plain LayerNorm
// backward of its norm1 / norm2 and the GELU backward of its Mlp.  Window 8x8, head_dim 32, fp32.
//
// One workgroup owns one (image, window, head): q, k, v of 64 x 32 and the 64 x 64 score matrix live in LDS, so the cyclic shift, the zero
// padding up to the window grid, the window partition and their inverses are index arithmetic on the way in and out - no rolled, padded or
// partitioned copy of a tensor and no score matrix reaches memory.  The two small products run on plain FMAs from LDS.
//
// The reference's frame is transposed (models/common.py:1317-1318): its window rows run along the map's W axis.  Token n of window (w1, w2):
// a1 = w1 * 8 + (n >> 3) along W, a2 = w2 * 8 + (n & 7) along H in the shifted, padded frame; it is the pixel x = (a1 + shift) % Wp,
// y = (a2 + shift) % Hp of the map, and a padding token (q = k = v = 0, still a key of every softmax) when x >= W or y >= H.
// Everything is summed in a fixed order: no float atomics in this file.
#include "common.h"

namespace somi {

constexpr int SW_N = 64;       // tokens per window
constexpr int SW_HD = 32;      // head dim
constexpr int SW_QS = 36;      // LDS row stride of q / k / v / dO: 16 rows 36 floats apart start in 16 different bank quads (ds_read_b128)
constexpr int SW_PS = 68;      // LDS row stride of the score matrix
constexpr int SW_BINS = 225;   // (2 * 8 - 1)^2 relative offsets
constexpr float SW_SCALE = 0.17677669529663687f;   // 32^-0.5

struct SwinGeo {
    int H, W, Hp, Wp, nW2, nWin, heads, shift;
};

static inline SwinGeo swin_geo(int H, int W, int heads, int shift) {
    SwinGeo g;
    g.H = H, g.W = W, g.heads = heads, g.shift = shift;
    g.Hp = (H + 7) / 8 * 8, g.Wp = (W + 7) / 8 * 8;
    g.nW2 = g.Hp / 8;
    g.nWin = (g.Wp / 8) * g.nW2;
    return g;
}

// spix[n]: the token's pixel index inside the batch (-1: padding), sid[n]: its region id (0 in an unshifted layer), sbias: the head's table column
__device__ __forceinline__ void swin_window_setup(const SwinGeo &g, const float *__restrict__ table, const int *__restrict__ ids, int b, int win,
                                                  int head, int *spix, int *sid, float *sbias) {
    const int tid = threadIdx.x;
    if (tid < SW_N) {
        const int a1 = (win / g.nW2) * 8 + (tid >> 3), a2 = (win % g.nW2) * 8 + (tid & 7);
        const int x = (a1 + g.shift) % g.Wp, y = (a2 + g.shift) % g.Hp;
        spix[tid] = (x < g.W && y < g.H) ? (b * g.H + y) * g.W + x : -1;
        sid[tid] = g.shift > 0 ? ids[a1 * g.Hp + a2] : 0;
    }
    if (tid < SW_BINS) sbias[tid] = table[tid * g.heads + head];
}

// rows of 32 floats of one head from a (pixels, cs) tensor into LDS (stride SW_QS), zeros for padding tokens
__device__ __forceinline__ void swin_load_rows(const float *__restrict__ src, long cs, int coff, const int *spix, float *dst, float mul) {
    for (int i = threadIdx.x; i < SW_N * 8; i += 256) {
        const int n = i >> 3, d = (i & 7) * 4;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (spix[n] >= 0) v = *reinterpret_cast<const f32x4 *>(src + (long)spix[n] * cs + coff + d) * mul;
        *reinterpret_cast<f32x4 *>(dst + n * SW_QS + d) = v;
    }
}

// acc[a][c] = sum_d A[ti * 4 + a][d] * Bm[tj + 16 * c][d]: the 4 x 4 tile of A Bm^T this thread owns (ti = tid >> 4, tj = tid & 15)
__device__ __forceinline__ void swin_tile_abt(const float *A, const float *Bm, float (&acc)[4][4]) {
    const int ti = threadIdx.x >> 4, tj = threadIdx.x & 15;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[a][c] = 0.f;
#pragma unroll 2
    for (int d = 0; d < SW_HD; d += 4) {
        f32x4 av[4], bv[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) av[a] = *reinterpret_cast<const f32x4 *>(A + (ti * 4 + a) * SW_QS + d);
#pragma unroll
        for (int c = 0; c < 4; ++c) bv[c] = *reinterpret_cast<const f32x4 *>(Bm + (tj + 16 * c) * SW_QS + d);
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int c = 0; c < 4; ++c)
                acc[a][c] += (av[a][0] * bv[c][0] + av[a][1] * bv[c][1]) + (av[a][2] * bv[c][2] + av[a][3] * bv[c][3]);
    }
}

// score = scaled q.k + relative-position bias (+ -100 across shift regions, models/common.py:1312), for this thread's tile
__device__ __forceinline__ void swin_add_bias_mask(float (&s)[4][4], const float *sbias, const int *sid) {
    const int ti = threadIdx.x >> 4, tj = threadIdx.x & 15;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int i = ti * 4 + a;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int j = tj + 16 * c;
            s[a][c] += sbias[((i >> 3) - (j >> 3) + 7) * 15 + ((i & 7) - (j & 7) + 7)];
            if (sid[i] != sid[j]) s[a][c] += -100.0f;
        }
    }
}

// out[r][d0 .. d0 + 8) = sum_m sp(r, m) * Bm[m][d0 ..], r = tid >> 2, d0 = (tid & 3) * 8; TRANS: sp read as its transpose (sp[m][r])
template <bool TRANS>
__device__ __forceinline__ void swin_p_times(const float *sp, const float *Bm, f32x4 &o0, f32x4 &o1) {
    const int r = threadIdx.x >> 2, d0 = (threadIdx.x & 3) * 8;
    o0 = o1 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
    for (int m = 0; m < SW_N; ++m) {
        const float p = TRANS ? sp[m * SW_PS + r] : sp[r * SW_PS + m];
        o0 += p * *reinterpret_cast<const f32x4 *>(Bm + m * SW_QS + d0);
        o1 += p * *reinterpret_cast<const f32x4 *>(Bm + m * SW_QS + d0 + 4);
    }
}

__device__ __forceinline__ float row16_max(float v) {            // over the 16 lanes that share a tile row (tj = lane & 15)
    for (int o = 8; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float row16_sum(float v) {
    for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ __launch_bounds__(256) void swin_attn_fwd_kernel(const float *__restrict__ qkv, const float *__restrict__ table,
                                                            const int *__restrict__ ids, float *__restrict__ o, float *__restrict__ lse,
                                                            SwinGeo g) {
    __shared__ __attribute__((aligned(16))) float sq[SW_N * SW_QS], sk[SW_N * SW_QS], sv[SW_N * SW_QS], sp[SW_N * SW_PS];
    __shared__ float sbias[SW_BINS];
    __shared__ int spix[SW_N], sid[SW_N];
    const int head = blockIdx.x % g.heads, win = (blockIdx.x / g.heads) % g.nWin, b = blockIdx.x / (g.heads * g.nWin);
    const int C = g.heads * SW_HD;
    swin_window_setup(g, table, ids, b, win, head, spix, sid, sbias);
    __syncthreads();
    swin_load_rows(qkv, 3L * C, head * SW_HD, spix, sq, SW_SCALE);     // q * scale first (models/common.py:1236), the bias after it
    swin_load_rows(qkv, 3L * C, C + head * SW_HD, spix, sk, 1.f);
    swin_load_rows(qkv, 3L * C, 2 * C + head * SW_HD, spix, sv, 1.f);
    __syncthreads();
    float s[4][4];
    swin_tile_abt(sq, sk, s);
    swin_add_bias_mask(s, sbias, sid);
    const int ti = threadIdx.x >> 4, tj = threadIdx.x & 15;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const float m = row16_max(fmaxf(fmaxf(s[a][0], s[a][1]), fmaxf(s[a][2], s[a][3])));
#pragma unroll
        for (int c = 0; c < 4; ++c) s[a][c] = expf(s[a][c] - m);
        const float l = row16_sum((s[a][0] + s[a][1]) + (s[a][2] + s[a][3]));
        const float inv = 1.0f / l;
#pragma unroll
        for (int c = 0; c < 4; ++c) sp[(ti * 4 + a) * SW_PS + tj + 16 * c] = s[a][c] * inv;
        if (lse && tj == 0) lse[(long)blockIdx.x * SW_N + ti * 4 + a] = m + logf(l);
    }
    __syncthreads();
    f32x4 o0, o1;
    swin_p_times<false>(sp, sv, o0, o1);
    const int r = threadIdx.x >> 2, d0 = (threadIdx.x & 3) * 8;
    if (spix[r] >= 0) {                                               // the crop: padding tokens write nothing
        float *dst = o + (long)spix[r] * C + head * SW_HD + d0;
        *reinterpret_cast<f32x4 *>(dst) = o0;
        *reinterpret_cast<f32x4 *>(dst + 4) = o1;
    }
}

// Recomputes P from q, k, the bias, the mask and the forward's log-sum-exp; dS = P * (dP - rowsum(P * dP)); dq = scale * dS k, dk = dS^T (scale q),
// dv = P^T dO.  part[workgroup][225]: the workgroup's dS summed per relative offset, every bin by the one thread that owns it.
__global__ __launch_bounds__(256) void swin_attn_bwd_kernel(const float *__restrict__ qkv, const float *__restrict__ table,
                                                            const int *__restrict__ ids, const float *__restrict__ dout,
                                                            const float *__restrict__ lse, float *__restrict__ dqkv, float *__restrict__ part,
                                                            SwinGeo g) {
    __shared__ __attribute__((aligned(16))) float sq[SW_N * SW_QS], sk[SW_N * SW_QS], sv[SW_N * SW_QS], sdo[SW_N * SW_QS], sp[SW_N * SW_PS];
    __shared__ float sbias[SW_BINS];
    __shared__ int spix[SW_N], sid[SW_N];
    const int head = blockIdx.x % g.heads, win = (blockIdx.x / g.heads) % g.nWin, b = blockIdx.x / (g.heads * g.nWin);
    const int C = g.heads * SW_HD;
    swin_window_setup(g, table, ids, b, win, head, spix, sid, sbias);
    __syncthreads();
    swin_load_rows(qkv, 3L * C, head * SW_HD, spix, sq, SW_SCALE);
    swin_load_rows(qkv, 3L * C, C + head * SW_HD, spix, sk, 1.f);
    swin_load_rows(qkv, 3L * C, 2 * C + head * SW_HD, spix, sv, 1.f);
    swin_load_rows(dout, C, head * SW_HD, spix, sdo, 1.f);             // padding tokens: their output was cropped, no gradient reaches them
    __syncthreads();
    float s[4][4], dp[4][4];
    swin_tile_abt(sq, sk, s);
    swin_add_bias_mask(s, sbias, sid);
    swin_tile_abt(sdo, sv, dp);
    const int ti = threadIdx.x >> 4, tj = threadIdx.x & 15;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const float l = lse[(long)blockIdx.x * SW_N + ti * 4 + a];
#pragma unroll
        for (int c = 0; c < 4; ++c) s[a][c] = expf(s[a][c] - l);
        const float D = row16_sum((s[a][0] * dp[a][0] + s[a][1] * dp[a][1]) + (s[a][2] * dp[a][2] + s[a][3] * dp[a][3]));
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            sp[(ti * 4 + a) * SW_PS + tj + 16 * c] = s[a][c];
            dp[a][c] = s[a][c] * (dp[a][c] - D);                      // dS
        }
    }
    __syncthreads();
    const int r = threadIdx.x >> 2, d0 = (threadIdx.x & 3) * 8;
    float *grow = spix[r] >= 0 ? dqkv + (long)spix[r] * 3 * C + head * SW_HD + d0 : nullptr;
    f32x4 o0, o1;
    swin_p_times<true>(sp, sdo, o0, o1);                              // dv
    if (grow) {
        *reinterpret_cast<f32x4 *>(grow + 2 * C) = o0;
        *reinterpret_cast<f32x4 *>(grow + 2 * C + 4) = o1;
    }
    __syncthreads();
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) sp[(ti * 4 + a) * SW_PS + tj + 16 * c] = dp[a][c];
    __syncthreads();
    swin_p_times<false>(sp, sk, o0, o1);                              // dq
    if (grow) {
        *reinterpret_cast<f32x4 *>(grow) = o0 * SW_SCALE;
        *reinterpret_cast<f32x4 *>(grow + 4) = o1 * SW_SCALE;
    }
    swin_p_times<true>(sp, sq, o0, o1);                               // dk (sq holds scale * q)
    if (grow) {
        *reinterpret_cast<f32x4 *>(grow + C) = o0;
        *reinterpret_cast<f32x4 *>(grow + C + 4) = o1;
    }
    if (threadIdx.x < SW_BINS) {                                      // this thread's bin: every (i, j) with i - j = (dr, dc), in a fixed order
        const int dr = threadIdx.x / 15 - 7, dc = threadIdx.x % 15 - 7;
        float acc = 0.f;
        for (int ri = max(0, dr); ri < min(8, 8 + dr); ++ri)
            for (int ci = max(0, dc); ci < min(8, 8 + dc); ++ci) acc += sp[(ri * 8 + ci) * SW_PS + (ri - dr) * 8 + (ci - dc)];
        part[(long)blockIdx.x * SW_BINS + threadIdx.x] = acc;
    }
}

// dtable[bin][head] += sum over (image, window) of part[(image, window)][head][bin]: 32 bins x 8 row groups per workgroup, a group walks every
// 8th partial row with 4 loads in flight, the 8 group sums are added in a fixed order
__global__ __launch_bounds__(256) void swin_table_grad_kernel(const float *__restrict__ part, int nbw, int heads, float *__restrict__ dtable) {
    __shared__ float l[256];
    const int bl = threadIdx.x & 31, grp = threadIdx.x >> 5;
    const int bin = blockIdx.x * 32 + bl, head = blockIdx.y;
    float a = 0.f;
    if (bin < SW_BINS) {
        const float *p = part + (long)head * SW_BINS + bin;
        const long rs = (long)heads * SW_BINS;
        int w = grp;
        for (; w + 3 * 8 < nbw; w += 4 * 8) {
            const float v0 = p[w * rs], v1 = p[(w + 8) * rs], v2 = p[(w + 16) * rs], v3 = p[(w + 24) * rs];
            a += (v0 + v1) + (v2 + v3);
        }
        for (; w < nbw; w += 8) a += p[w * rs];
    }
    l[threadIdx.x] = a;
    __syncthreads();
    if (grp != 0 || bin >= SW_BINS) return;
    float s = 0.f;
    for (int k = 0; k < 8; ++k) s += l[k * 32 + bl];
    dtable[bin * heads + head] += s;
}

// y = LN(u) * gamma + beta: du = rstd * (g - mean(g) - xhat * mean(g * xhat)) (+ add), g = dy * gamma; one wave per pixel row; per-workgroup
// partial sums of dgamma = sum dy * xhat and dbeta = sum dy go to part[blk][2][C] (ln_gelu_bwd_kernel of dcnv3_module_bwd.hip without the GELU)
__global__ __launch_bounds__(256) void ln_bwd_kernel(const float *__restrict__ u, const float *__restrict__ gamma, float eps,
                                                     const float *__restrict__ dy, const float *__restrict__ add, float *__restrict__ du,
                                                     float *__restrict__ part, long npix, int C) {
    extern __shared__ float sm[];                                   // [4 waves][2][C]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float *mg = sm + (size_t)wave * 2 * C, *mb = mg + C;
    for (int c = lane; c < C; c += 64) { mg[c] = 0.f; mb[c] = 0.f; }
    const long wave_id = blockIdx.x * 4L + wave, nwave = (long)gridDim.x * 4;
    for (long p = wave_id; p < npix; p += nwave) {
        const float *ur = u + p * C, *dr = dy + p * C;
        float s = 0.f;
        for (int c = lane * 4; c < C; c += 256) {
            const f32x4 v = *reinterpret_cast<const f32x4 *>(ur + c);
            s += (v[0] + v[1]) + (v[2] + v[3]);
        }
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        const float mean = s / (float)C;
        float q = 0.f;
        for (int c = lane * 4; c < C; c += 256) {
            const f32x4 v = *reinterpret_cast<const f32x4 *>(ur + c) - mean;
            q += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
        }
        for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
        const float rstd = rsqrtf(q / (float)C + eps);
        float sg = 0.f, sgx = 0.f;
        for (int c = lane * 4; c < C; c += 256) {
            const f32x4 xh = (*reinterpret_cast<const f32x4 *>(ur + c) - mean) * rstd;
            const f32x4 gm = *reinterpret_cast<const f32x4 *>(gamma + c);
            const f32x4 d = *reinterpret_cast<const f32x4 *>(dr + c);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                mg[c + e] += d[e] * xh[e];                            // this lane owns columns c..c+3 of its wave's partial
                mb[c + e] += d[e];
                const float gv = d[e] * gm[e];
                sg += gv;
                sgx += gv * xh[e];
            }
        }
        for (int o = 32; o > 0; o >>= 1) { sg += __shfl_xor(sg, o); sgx += __shfl_xor(sgx, o); }
        const float m1 = sg / (float)C, m2 = sgx / (float)C;
        for (int c = lane * 4; c < C; c += 256) {
            const f32x4 xh = (*reinterpret_cast<const f32x4 *>(ur + c) - mean) * rstd;
            const f32x4 gm = *reinterpret_cast<const f32x4 *>(gamma + c);
            const f32x4 d = *reinterpret_cast<const f32x4 *>(dr + c);
            f32x4 o = (d * gm - m1 - xh * m2) * rstd;
            if (add) o += *reinterpret_cast<const f32x4 *>(add + p * C + c);
            *reinterpret_cast<f32x4 *>(du + p * C + c) = o;
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < 2 * C; c += 256)                    // fixed order over the 4 waves
        part[(size_t)blockIdx.x * 2 * C + c] = (sm[c] + sm[2 * C + c]) + (sm[4 * C + c] + sm[6 * C + c]);
}

// column sums of the nblk partial rows: 16 columns x 16 row groups per workgroup, the 16 group sums added in a fixed order
__global__ __launch_bounds__(256) void ln_bwd_param_kernel(const float *__restrict__ part, int nblk, int C, float *dgamma, float *dbeta) {
    __shared__ float l[256];
    const int cl = threadIdx.x & 15, grp = threadIdx.x >> 4;
    const int c = blockIdx.x * 16 + cl;
    float a = 0.f;
    if (c < 2 * C)
        for (int b = grp; b < nblk; b += 16) a += part[(size_t)b * 2 * C + c];
    l[threadIdx.x] = a;
    __syncthreads();
    if (grp != 0 || c >= 2 * C) return;
    float s = 0.f;
    for (int k = 0; k < 16; ++k) s += l[k * 16 + cl];
    if (c < C) dgamma[c] += s;
    else dbeta[c - C] += s;
}

__global__ __launch_bounds__(256) void gelu_bwd_kernel(const float *__restrict__ u, const float *__restrict__ dy, float *__restrict__ du, long n4) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const f32x4 v = reinterpret_cast<const f32x4 *>(u)[i], d = reinterpret_cast<const f32x4 *>(dy)[i];
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = d[e] * gelu_grad(v[e]);
        reinterpret_cast<f32x4 *>(du)[i] = o;
    }
}

static inline int ln_bwd_blocks(long npix) {
    const long g = (npix + 3) / 4;
    return (int)(g < 1 ? 1 : (g > 1024 ? 1024 : g));
}

static int swin_check(const char *who, const void *qkv, const void *table, const int *ids, int B, int H, int W, int heads, int shift) {
    SOMI_REQUIRE(qkv && table && B > 0 && H > 0 && W > 0 && heads > 0, SOMI_EINVAL, "%s: bad arguments (NULL pointer or empty shape)", who);
    SOMI_REQUIRE(aligned16(qkv), SOMI_EINVAL, "%s: qkv not 16-byte aligned", who);
    SOMI_REQUIRE(shift == 0 || shift == 4, SOMI_EINVAL, "%s: shift %d (0 or 4: window 8)", who, shift);
    SOMI_REQUIRE(shift == 0 || ids, SOMI_EINVAL, "%s: a shifted layer needs the region-id map", who);
    const SwinGeo g = swin_geo(H, W, heads, shift);
    SOMI_REQUIRE((long)B * g.nWin * heads < (1L << 31) / SW_BINS && (long)B * H * W * 3 * heads * SW_HD < (1L << 40), SOMI_EINVAL,
                 "%s: shape too large", who);
    return 0;
}

}  // namespace somi

using namespace somi;

extern "C" int somi_swin_attention_f32(const float *qkv, const float *table, const int32_t *region_ids, int B, int H, int W, int C, int heads,
                                       int shift, float *o, float *lse, somi_stream_t stream) {
    SOMI_REQUIRE(heads > 0 && C == heads * SW_HD, SOMI_ENOTIMPL, "swin attention: head_dim 32 only (C = %d, heads = %d)", C, heads);
    if (int rc = swin_check("swin attention", qkv, table, region_ids, B, H, W, heads, shift)) return rc;
    SOMI_REQUIRE(o && aligned16(o), SOMI_EINVAL, "swin attention: output NULL or not 16-byte aligned");
    const SwinGeo g = swin_geo(H, W, heads, shift);
    hipLaunchKernelGGL(swin_attn_fwd_kernel, dim3(B * g.nWin * heads), dim3(256), 0, (hipStream_t)stream, qkv, table, region_ids, o, lse, g);
    return launch_status("somi_swin_attention_f32");
}

extern "C" size_t somi_swin_attention_lse_floats(int B, int H, int W, int heads) {
    if (B <= 0 || H <= 0 || W <= 0 || heads <= 0) return 0;
    return (size_t)B * swin_geo(H, W, heads, 0).nWin * heads * SW_N;
}

extern "C" size_t somi_swin_attention_bwd_workspace_floats(int B, int H, int W, int heads) {
    if (B <= 0 || H <= 0 || W <= 0 || heads <= 0) return 0;
    return (size_t)B * swin_geo(H, W, heads, 0).nWin * heads * SW_BINS;
}

extern "C" int somi_swin_attention_backward_f32(const float *qkv, const float *table, const int32_t *region_ids, const float *dout,
                                                const float *lse, int B, int H, int W, int C, int heads, int shift, float *dqkv,
                                                float *dtable_accumulate, float *workspace, somi_stream_t stream) {
    SOMI_REQUIRE(heads > 0 && C == heads * SW_HD, SOMI_ENOTIMPL, "swin attention backward: head_dim 32 only (C = %d, heads = %d)", C, heads);
    if (int rc = swin_check("swin attention backward", qkv, table, region_ids, B, H, W, heads, shift)) return rc;
    SOMI_REQUIRE(dout && lse && dqkv && dtable_accumulate && workspace, SOMI_EINVAL, "swin attention backward: NULL pointer");
    SOMI_REQUIRE(aligned16(dout) && aligned16(dqkv), SOMI_EINVAL, "swin attention backward: dout / dqkv not 16-byte aligned");
    const SwinGeo g = swin_geo(H, W, heads, shift);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(swin_attn_bwd_kernel, dim3(B * g.nWin * heads), dim3(256), 0, s, qkv, table, region_ids, dout, lse, dqkv, workspace, g);
    hipLaunchKernelGGL(swin_table_grad_kernel, dim3(cdiv(SW_BINS, 32), heads), dim3(256), 0, s, workspace, B * g.nWin, heads, dtable_accumulate);
    return launch_status("somi_swin_attention_backward_f32");
}

extern "C" size_t somi_layernorm_bwd_workspace_floats(long npix, int C) {
    return npix > 0 && C > 0 ? (size_t)ln_bwd_blocks(npix) * 2 * (size_t)C : 0;
}

extern "C" int somi_layernorm_bwd_nhwc_f32(const float *u, const float *gamma, float eps, const float *dy, const float *add, float *du,
                                           float *dgamma_accumulate, float *dbeta_accumulate, float *workspace, long npix, int C,
                                           somi_stream_t stream) {
    SOMI_REQUIRE(u && gamma && dy && du && dgamma_accumulate && dbeta_accumulate && workspace && npix > 0 && C > 0 && C % 4 == 0 && aligned16(u) &&
                     aligned16(dy) && aligned16(du) && aligned16(gamma) && (!add || aligned16(add)), SOMI_EINVAL,
                 "layernorm backward: bad arguments (C %% 4, 16 B alignment)");
    SOMI_REQUIRE((size_t)C * 8 * sizeof(float) <= 64 * 1024, SOMI_ENOTIMPL, "layernorm backward: C up to 2048");
    const int nblk = ln_bwd_blocks(npix);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(ln_bwd_kernel, dim3(nblk), dim3(256), (size_t)C * 8 * sizeof(float), s, u, gamma, eps, dy, add, du, workspace, npix, C);
    hipLaunchKernelGGL(ln_bwd_param_kernel, dim3(cdiv(2L * C, 16)), dim3(256), 0, s, workspace, nblk, C, dgamma_accumulate, dbeta_accumulate);
    return launch_status("somi_layernorm_bwd_nhwc_f32");
}

extern "C" int somi_gelu_bwd_f32(const float *u, const float *dy, float *du, long n, somi_stream_t stream) {
    SOMI_REQUIRE(u && dy && du && n > 0 && n % 4 == 0 && aligned16(u) && aligned16(dy) && aligned16(du), SOMI_EINVAL,
                 "gelu backward: bad arguments (n %% 4, 16 B alignment)");
    const long g = (n / 4 + 255) / 256;
    hipLaunchKernelGGL(gelu_bwd_kernel, dim3((unsigned)(g > 4096 ? 4096 : g)), dim3(256), 0, (hipStream_t)stream, u, dy, du, n / 4);
    return launch_status("somi_gelu_bwd_f32");
}
