// Multi-head spatial self-attention of PSA (models/common.py:7203-7230, AttentionPSA), NHWC fp32, flash style.
//
// The qkv Conv's output is read in place: pixel stride qkv_cs, channel offset qkv_coff, and per head h the channels h*128 + [0,32) are
// q, h*128 + [32,64) k and h*128 + [64,128) v (key_dim 32 and head_dim 64 are compile-time constants).  With N = H*W tokens per image,
// P = softmax_j(q_i . k_j / sqrt(32)) and o[h*64 + d, i] = sum_j P[i,j] v[d, j].  The N x N matrix never reaches memory: a workgroup of
// four waves owns 128 rows (32 per wave) and walks 32-row tiles of the other side, staged in LDS, with an online max / sum.
//
// Arithmetic: v_mfma_f32_32x32x2_f32 (exact fp32 products, as in conv_igemm.hip).  Operand A's lane l carries row l%32, operand B's lane
// l column l%32, both at k index l/32; the accumulator's register e holds row 8(e/4) + 4(l/32) + e%4 of column l%32.  Every product is
// arranged so that the 32 rows a wave owns sit on the lanes: a row's softmax statistics are then 16 registers and one swap with lane
// l^32.  A chain's k order is free as long as both operands follow it, so the second product of a pair takes k step t from register t
// of the first product's accumulator (k index 8(t/4) + 4(l/32) + t%4): probabilities never leave the registers.
//
// Backward (recomputes P from the saved log-sum-exp): one kernel owns query tiles and writes dq and D_i = sum_d dO.O of its rows; a
// second owns key tiles and writes dk and dv (plus an optional addend, pe's data gradient).  Fixed-order sums, no float atomics: every
// launch is bit-identical.
#include "common.h"

namespace somi {
namespace {

constexpr int KD = 32, HD = 64, QKV_H = 2 * KD + HD;              // per head: q 32 | k 32 | v 64 channels
constexpr int TILE = 32, WAVES = 4, THREADS = 64 * WAVES, ROWS_WG = TILE * WAVES;
constexpr int KLD = KD + 4, VLD = HD + 4;                         // padded LDS row strides (floats)
constexpr float LOG2E = 1.4426950408889634f, LN2 = 0.6931471805599453f;
constexpr float SCALE = 0.17677669529663687f;                     // key_dim ** -0.5

struct AttnArgs {
    const float *qkv, *o, *dout, *lse, *dv_add;
    float *out, *lse_out, *v_out, *dqkv, *dsum;
    int qkv_cs, qkv_coff, o_cs, o_coff, do_cs, do_coff, g_cs, g_coff, B, N, heads;
};

__device__ __forceinline__ f32x16 mfma(float a, float b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }

__device__ __forceinline__ f32x4 ld4(const float *p) { return *reinterpret_cast<const f32x4 *>(p); }
__device__ __forceinline__ void st4(float *p, f32x4 v) { *reinterpret_cast<f32x4 *>(p) = v; }

// k index of step t for lane half hh (t < 16 per 32-wide chain): register t of an accumulator holds that row
__device__ __forceinline__ int kperm(int t, int hh) { return 8 * (t >> 2) + 4 * hh + (t & 3); }

// stages rows [r0, r0 + 32) of a 32-wide and a 64-wide channel slice (zero past N) into LDS
__device__ __forceinline__ void stage_tile(const float *src32, const float *src64, size_t cs32, size_t cs64, int r0, int N, float *s32,
                                           float *s64, int tid) {
    {
        const int r = tid >> 3, c = (tid & 7) * 4;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (r0 + r < N) v = ld4(src32 + (size_t)(r0 + r) * cs32 + c);
        st4(s32 + r * KLD + c, v);
    }
#pragma unroll
    for (int i = tid; i < TILE * HD / 4; i += THREADS) {
        const int r = i >> 4, c = (i & 15) * 4;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (r0 + r < N) v = ld4(src64 + (size_t)(r0 + r) * cs64 + c);
        st4(s64 + r * VLD + c, v);
    }
}

__global__ __launch_bounds__(THREADS) void attn_fwd_kernel(AttnArgs a) {
    __shared__ float sk[TILE * KLD];
    __shared__ float sv[TILE * VLD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hh = lane >> 5, r32 = lane & 31;
    const int head = blockIdx.y, b = blockIdx.z, N = a.N;
    const size_t img = (size_t)b * N, cs = (size_t)a.qkv_cs;
    const float *base = a.qkv + img * cs + a.qkv_coff + head * QKV_H;
    const int r0 = blockIdx.x * ROWS_WG;
    if (a.v_out) {                                                // v of this workgroup's rows, contiguous (B, N, heads*64): pe's input
        const size_t vcs = (size_t)a.heads * HD;
        for (int i = tid; i < ROWS_WG * HD / 4; i += THREADS) {
            const int r = r0 + i / (HD / 4), c = (i % (HD / 4)) * 4;
            if (r < N) st4(a.v_out + (img + r) * vcs + head * HD + c, ld4(base + r * cs + 2 * KD + c));
        }
    }
    const int q = r0 + wave * TILE + r32;
    const bool live = r0 + wave * TILE < N;
    float qr[16];                                                 // q * scale * log2(e): the scores come out in the exp2 domain
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (q < N) v = ld4(base + q * cs + 8 * g + 4 * hh);
#pragma unroll
        for (int j = 0; j < 4; ++j) qr[4 * g + j] = v[j] * (SCALE * LOG2E);
    }
    f32x16 o0, o1;
#pragma unroll
    for (int e = 0; e < 16; ++e) o0[e] = o1[e] = 0.f;
    float m = -INFINITY, l = 0.f;
    const int nkt = (N + TILE - 1) / TILE;
    for (int kt = 0; kt < nkt; ++kt) {
        __syncthreads();
        stage_tile(base + KD, base + 2 * KD, cs, cs, kt * TILE, N, sk, sv, tid);
        __syncthreads();
        if (!live) continue;
        f32x16 s;                                                 // S^T[key][query] = K Q^T
#pragma unroll
        for (int e = 0; e < 16; ++e) s[e] = 0.f;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 kv = ld4(sk + r32 * KLD + 8 * g + 4 * hh);
#pragma unroll
            for (int j = 0; j < 4; ++j) s = mfma(kv[j], qr[4 * g + j], s);
        }
        float tmax = -INFINITY;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            if (kt * TILE + kperm(e, hh) >= N) s[e] = -INFINITY;
            tmax = fmaxf(tmax, s[e]);
        }
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32));                 // key 0 of every tile is valid: tmax is finite
        const float mn = fmaxf(m, tmax), alpha = exp2f(m - mn);
        float ps = 0.f;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            s[e] = exp2f(s[e] - mn);
            ps += s[e];
        }
        ps += __shfl_xor(ps, 32);
        l = l * alpha + ps;
        m = mn;
        o0 *= alpha;
        o1 *= alpha;
#pragma unroll
        for (int t = 0; t < 16; ++t) {                            // O^T[d][query] += V^T P^T, k step t = register t
            const float *vr = sv + kperm(t, hh) * VLD + r32;
            o0 = mfma(vr[0], s[t], o0);
            o1 = mfma(vr[32], s[t], o1);
        }
    }
    if (!live || q >= N) return;
    const float inv = 1.0f / l;
    float *op = a.out + (img + q) * (size_t)a.o_cs + a.o_coff + head * HD;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const f32x4 v0 = {o0[4 * g] * inv, o0[4 * g + 1] * inv, o0[4 * g + 2] * inv, o0[4 * g + 3] * inv};
        const f32x4 v1 = {o1[4 * g] * inv, o1[4 * g + 1] * inv, o1[4 * g + 2] * inv, o1[4 * g + 3] * inv};
        st4(op + 8 * g + 4 * hh, v0);
        st4(op + 32 + 8 * g + 4 * hh, v1);
    }
    if (a.lse_out && hh == 0) a.lse_out[((size_t)b * a.heads + head) * N + q] = (m + log2f(l)) * LN2;
}

// query tiles: dq = scale * sum_j dS[i,j] k_j, dS = P (dP - D_i), dP = dO v^T; also leaves D_i for the key-tile kernel
__global__ __launch_bounds__(THREADS) void attn_bwd_dq_kernel(AttnArgs a) {
    __shared__ float sk[TILE * KLD];
    __shared__ float sv[TILE * VLD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hh = lane >> 5, r32 = lane & 31;
    const int head = blockIdx.y, b = blockIdx.z, N = a.N;
    const size_t img = (size_t)b * N, cs = (size_t)a.qkv_cs, row = ((size_t)b * a.heads + head) * N;
    const float *base = a.qkv + img * cs + a.qkv_coff + head * QKV_H;
    const int r0 = blockIdx.x * ROWS_WG, q = r0 + wave * TILE + r32;
    const bool live = r0 + wave * TILE < N;
    float qr[16], dor[32], lse2 = 0.f, dd = 0.f;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (q < N) v = ld4(base + q * cs + 8 * g + 4 * hh);
#pragma unroll
        for (int j = 0; j < 4; ++j) qr[4 * g + j] = v[j] * (SCALE * LOG2E);
    }
#pragma unroll
    for (int g = 0; g < 8; ++g) {
        f32x4 d4 = {0.f, 0.f, 0.f, 0.f}, o4 = d4;
        if (q < N) {
            d4 = ld4(a.dout + (img + q) * (size_t)a.do_cs + a.do_coff + head * HD + 8 * g + 4 * hh);
            o4 = ld4(a.o + (img + q) * (size_t)a.o_cs + a.o_coff + head * HD + 8 * g + 4 * hh);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            dor[4 * g + j] = d4[j];
            dd = fmaf(d4[j], o4[j], dd);
        }
    }
    dd += __shfl_xor(dd, 32);
    if (q < N) {
        lse2 = a.lse[row + q] * LOG2E;
        if (hh == 0) a.dsum[row + q] = dd;
    }
    f32x16 dq;
#pragma unroll
    for (int e = 0; e < 16; ++e) dq[e] = 0.f;
    const int nkt = (N + TILE - 1) / TILE;
    for (int kt = 0; kt < nkt; ++kt) {
        __syncthreads();
        stage_tile(base + KD, base + 2 * KD, cs, cs, kt * TILE, N, sk, sv, tid);
        __syncthreads();
        if (!live) continue;
        f32x16 s, dp;                                             // S^T = K Q^T, dP^T = V dO^T: lane = query, register = key
#pragma unroll
        for (int e = 0; e < 16; ++e) s[e] = dp[e] = 0.f;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 kv = ld4(sk + r32 * KLD + 8 * g + 4 * hh);
#pragma unroll
            for (int j = 0; j < 4; ++j) s = mfma(kv[j], qr[4 * g + j], s);
        }
#pragma unroll
        for (int g = 0; g < 8; ++g) {
            const f32x4 vv = ld4(sv + r32 * VLD + 8 * g + 4 * hh);
#pragma unroll
            for (int j = 0; j < 4; ++j) dp = mfma(vv[j], dor[4 * g + j], dp);
        }
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const float p = (q < N && kt * TILE + kperm(e, hh) < N) ? exp2f(s[e] - lse2) : 0.f;
            s[e] = p * (dp[e] - dd);
        }
#pragma unroll
        for (int t = 0; t < 16; ++t) dq = mfma(sk[kperm(t, hh) * KLD + r32], s[t], dq);   // dQ^T[d][query] += K^T dS^T
    }
    if (!live || q >= N) return;
    float *gp = a.dqkv + (img + q) * (size_t)a.g_cs + a.g_coff + head * QKV_H;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const f32x4 v = {dq[4 * g] * SCALE, dq[4 * g + 1] * SCALE, dq[4 * g + 2] * SCALE, dq[4 * g + 3] * SCALE};
        st4(gp + 8 * g + 4 * hh, v);
    }
}

// key tiles: dk = scale * sum_i dS[i,j] q_i, dv = sum_i P[i,j] dO_i (+ dv_add)
__global__ __launch_bounds__(THREADS) void attn_bwd_dkv_kernel(AttnArgs a) {
    __shared__ float sq[TILE * KLD];
    __shared__ float sdo[TILE * VLD];
    __shared__ float sl[TILE], sd[TILE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hh = lane >> 5, r32 = lane & 31;
    const int head = blockIdx.y, b = blockIdx.z, N = a.N;
    const size_t img = (size_t)b * N, cs = (size_t)a.qkv_cs, row = ((size_t)b * a.heads + head) * N;
    const float *base = a.qkv + img * cs + a.qkv_coff + head * QKV_H;
    const float *dobase = a.dout + img * (size_t)a.do_cs + a.do_coff + head * HD;
    const int r0 = blockIdx.x * ROWS_WG, key = r0 + wave * TILE + r32;
    const bool live = r0 + wave * TILE < N;
    float kr[16], vr[32];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (key < N) v = ld4(base + key * cs + KD + 8 * g + 4 * hh);
#pragma unroll
        for (int j = 0; j < 4; ++j) kr[4 * g + j] = v[j];
    }
#pragma unroll
    for (int g = 0; g < 8; ++g) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (key < N) v = ld4(base + key * cs + 2 * KD + 8 * g + 4 * hh);
#pragma unroll
        for (int j = 0; j < 4; ++j) vr[4 * g + j] = v[j];
    }
    f32x16 dk, dv0, dv1;
#pragma unroll
    for (int e = 0; e < 16; ++e) dk[e] = dv0[e] = dv1[e] = 0.f;
    const int nqt = (N + TILE - 1) / TILE;
    for (int qt = 0; qt < nqt; ++qt) {
        __syncthreads();
        stage_tile(base, dobase, cs, (size_t)a.do_cs, qt * TILE, N, sq, sdo, tid);
        if (tid < TILE) {
            const int qq = qt * TILE + tid;
            sl[tid] = qq < N ? a.lse[row + qq] * LOG2E : 0.f;
            sd[tid] = qq < N ? a.dsum[row + qq] : 0.f;
        }
        __syncthreads();
        if (!live) continue;
        f32x16 s, dp;                                             // S = Q K^T, dP = dO V^T: lane = key, register = query
#pragma unroll
        for (int e = 0; e < 16; ++e) s[e] = dp[e] = 0.f;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 qv = ld4(sq + r32 * KLD + 8 * g + 4 * hh);
#pragma unroll
            for (int j = 0; j < 4; ++j) s = mfma(qv[j], kr[4 * g + j], s);
        }
#pragma unroll
        for (int g = 0; g < 8; ++g) {
            const f32x4 dv4 = ld4(sdo + r32 * VLD + 8 * g + 4 * hh);
#pragma unroll
            for (int j = 0; j < 4; ++j) dp = mfma(dv4[j], vr[4 * g + j], dp);
        }
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int ql = kperm(e, hh);
            s[e] = qt * TILE + ql < N ? exp2f(s[e] * (SCALE * LOG2E) - sl[ql]) : 0.f;
        }
#pragma unroll
        for (int t = 0; t < 16; ++t) {                            // dV^T[d][key] += dO^T P
            const float *dr = sdo + kperm(t, hh) * VLD + r32;
            dv0 = mfma(dr[0], s[t], dv0);
            dv1 = mfma(dr[32], s[t], dv1);
        }
#pragma unroll
        for (int e = 0; e < 16; ++e) s[e] *= dp[e] - sd[kperm(e, hh)];
#pragma unroll
        for (int t = 0; t < 16; ++t) dk = mfma(sq[kperm(t, hh) * KLD + r32], s[t], dk);   // dK^T[d][key] += Q^T dS
    }
    if (!live || key >= N) return;
    float *gp = a.dqkv + (img + key) * (size_t)a.g_cs + a.g_coff + head * QKV_H;
    const float *add = a.dv_add ? a.dv_add + (img + key) * (size_t)(a.heads * HD) + head * HD : nullptr;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int d = 8 * g + 4 * hh;
        const f32x4 k4 = {dk[4 * g] * SCALE, dk[4 * g + 1] * SCALE, dk[4 * g + 2] * SCALE, dk[4 * g + 3] * SCALE};
        f32x4 v0 = {dv0[4 * g], dv0[4 * g + 1], dv0[4 * g + 2], dv0[4 * g + 3]};
        f32x4 v1 = {dv1[4 * g], dv1[4 * g + 1], dv1[4 * g + 2], dv1[4 * g + 3]};
        if (add) {
            v0 += ld4(add + d);
            v1 += ld4(add + 32 + d);
        }
        st4(gp + KD + d, k4);
        st4(gp + 2 * KD + d, v0);
        st4(gp + 2 * KD + 32 + d, v1);
    }
}

}  // namespace
}  // namespace somi

using namespace somi;

extern "C" int somi_psa_attention_f32(const float *qkv, int qkv_cs, int qkv_coff, int B, int N, int heads, float *o, int o_cs, int o_coff,
                                      float *lse, float *v_out, somi_stream_t stream) {
    SOMI_REQUIRE(B > 0 && N > 0 && heads > 0 && heads <= 65535 && B <= 65535, SOMI_EINVAL, "psa attention: bad sizes");
    SOMI_REQUIRE_SLICES("psa attention", {"qkv", qkv, qkv_cs, qkv_coff, heads * QKV_H}, {"o", o, o_cs, o_coff, heads * HD});
    SOMI_REQUIRE((!lse || aligned16(lse)) && (!v_out || aligned16(v_out)), SOMI_EINVAL, "psa attention: lse and v_out must be 16-byte aligned");
    AttnArgs a = {};
    a.qkv = qkv; a.qkv_cs = qkv_cs; a.qkv_coff = qkv_coff; a.out = o; a.o_cs = o_cs; a.o_coff = o_coff; a.lse_out = lse; a.v_out = v_out;
    a.B = B; a.N = N; a.heads = heads;
    hipLaunchKernelGGL(attn_fwd_kernel, dim3(cdiv(N, ROWS_WG), heads, B), dim3(THREADS), 0, (hipStream_t)stream, a);
    return launch_status("somi_psa_attention_f32");
}

extern "C" int somi_psa_attention_backward_f32(const float *qkv, int qkv_cs, int qkv_coff, const float *o, int o_cs, int o_coff,
                                               const float *dout, int do_cs, int do_coff, const float *lse, int B, int N, int heads,
                                               float *dqkv, int g_cs, int g_coff, const float *dv_add, float *workspace,
                                               somi_stream_t stream) {
    SOMI_REQUIRE(B > 0 && N > 0 && heads > 0 && heads <= 65535 && B <= 65535, SOMI_EINVAL, "psa attention backward: bad sizes");
    SOMI_REQUIRE_SLICES("psa attention backward", {"qkv", qkv, qkv_cs, qkv_coff, heads * QKV_H}, {"o", o, o_cs, o_coff, heads * HD},
                        {"dout", dout, do_cs, do_coff, heads * HD}, {"dqkv", dqkv, g_cs, g_coff, heads * QKV_H});
    SOMI_REQUIRE(lse && workspace && (!dv_add || aligned16(dv_add)), SOMI_EINVAL, "psa attention backward: needs lse, workspace and a 16-byte aligned dv_add");
    AttnArgs a = {};
    a.qkv = qkv; a.qkv_cs = qkv_cs; a.qkv_coff = qkv_coff; a.o = o; a.o_cs = o_cs; a.o_coff = o_coff; a.dout = dout; a.do_cs = do_cs;
    a.do_coff = do_coff; a.lse = lse; a.dqkv = dqkv; a.g_cs = g_cs; a.g_coff = g_coff; a.dv_add = dv_add; a.dsum = workspace;
    a.B = B; a.N = N; a.heads = heads;
    const dim3 grid(cdiv(N, ROWS_WG), heads, B);
    hipLaunchKernelGGL(attn_bwd_dq_kernel, grid, dim3(THREADS), 0, (hipStream_t)stream, a);
    if (int rc = launch_status("somi_psa_attention_backward_f32 (dq)")) return rc;
    hipLaunchKernelGGL(attn_bwd_dkv_kernel, grid, dim3(THREADS), 0, (hipStream_t)stream, a);
    return launch_status("somi_psa_attention_backward_f32 (dk, dv)");
}
