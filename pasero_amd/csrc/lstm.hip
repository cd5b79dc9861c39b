// The LSTM recurrence of `hybrid_transformer`'s decoder (pasero/models/hybrid.py: nn.LSTM, one layer, batch first).
//
// The input-side product  gx = LN(x) W_ih^T + b_ih  over all B T rows is an ordinary GEMM done by the caller; what is left is
// serial in t:
//     pre_t = gx[:, t] + b_hh + h_{t-1} W_hh^T                      W_hh [4H][H], gate order i, f, g, o
//     i, f, o = sigmoid(.)   g = tanh(.)   c_t = f c_{t-1} + i g    h_t = o tanh(c_t)
// pk_lstm_fwd walks t on the host, ONE launch per step (a dependent launch boundary costs 1-2 us; nothing here spins on
// another workgroup).  A step launch tiles (16 rows of B) x (16 hidden units j): one wave per tile accumulates the four
// gate columns {j, H+j, 2H+j, 3H+j} of h_{t-1} W_hh^T over K = H — v_mfma_f32_16x16x32 for the 16-bit types, h fragments and
// W_hh fragments straight from global memory in MFMA layout (16 B per lane: k is the contiguous index of both), plain FMA
// in the same lane layout for fp32 — and does the whole cell in its epilogue.  c_t is rounded to the storage type BEFORE
// tanh(c_t), and h_t, c_t and the activated gates are stored rounded, so step t+1 reads exactly what a caller would pass
// back in: a T-step call is bit for bit T one-step calls.  An output element is one dot product in a fixed k order that no
// other row enters: a row's result does not depend on the rows that share the call.
// No scratch: h_{t-1} is y[:, t-1] and c_{t-1} is c[:, t-1] (h0 / c0, or zero, at t = 0).
//
// pk_lstm_bwd walks t = T-1 .. 0, one launch per step on the same tiling:
//     dh = dy[:, t] + dG_{t+1} W_hh   (K = 4H; W_hh transposed once per call into scratch so that k is contiguous again)
//     dc = dc_carry + dh o (1 - tanh^2 c_t)     dG_t = (dc g i(1-i), dc c_{t-1} f(1-f), dc i (1-g^2), dh tanh(c_t) o(1-o))
//     dc_carry = dc f                          (fp32, in scratch; element (row, j) is owned by the same lane at every step)
// dG is written in the storage type [B][T][4H]; d gx = dG, and dW_hh / db_hh are (B T)-row products of dG done by the caller.
// Gradients towards h0 / c0 are not produced.
#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(4))) float lstm_f32x4;

struct LstmFwdArgs {
    const void *gx, *whh, *bhh, *hprev, *cprev;  // hprev / cprev: rows of h_{t-1} / c_{t-1} or null (zero state)
    void *y, *c, *gates, *hT, *cT;               // already offset to step t; hT / cT null except at the last step
    long long gx_ldb, hprev_ld, cprev_ld, out_ld;  // row strides in elements (out_ld: T*H for y and c, gates use 4x)
    int B, H;
};

struct LstmBwdArgs {
    const void *dy, *dg_next, *whhT, *gates, *c, *cprev;  // offset to step t; dg_next null at t = T-1; cprev null: zero
    void* dg;
    float* dc;                                            // [B][H] carry
    long long ld, cprev_ld;                               // ld = T*H (dy, c); gates / dG rows are 4 ld apart
    int B, H, first;                                      // first: t = T-1 (the carry starts at zero)
};

// (fp32 keeps the library exp: parity with an fp64 restatement to a few 1e-7; the 16-bit types round far coarser)
template <typename T> __device__ __forceinline__ float sigmoid_f(float x) {
    if constexpr (sizeof(T) == 2) return 1.f / (1.f + __expf(-x));
    else return 1.f / (1.f + expf(-x));
}

// acc[g][reg] += sum_k A[row0 + 4 (lane>>4) + reg][k] * W[(g * GS + col0 + (lane&15))][k],  k < K; A rows >= rows read as 0.
// 16-bit: the 16x16x32 MFMA (A lane map: row lane&15, k 8 (lane>>4) + e; C map: col lane&15, row 4 (lane>>4) + reg).
template <typename T>
__device__ __forceinline__ void tile_gates(const T* __restrict__ A, long long lda, int rows, int row0, const T* __restrict__ W,
                                           int K, long long gate_stride, int col0, lstm_f32x4 (&acc)[4]) {
    const int lane = threadIdx.x & 63;
    if constexpr (sizeof(T) == 2) {
        const int ar = row0 + (lane & 15), kq = 8 * (lane >> 4);
        const bool live = ar < rows;
        const T* ap = A + (long long)ar * lda + kq;
        const T* wp = W + (long long)(col0 + (lane & 15)) * K + kq;
        // U k-steps per pass: their loads leave together, so a pass waits on memory once per 32 U of k, not once per 32
        constexpr int U = 4;
        typedef typename H16<T>::vec V;
        for (int k = 0; k < K; k += 32 * U) {
            uint4 fa[U], fb[U][4];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int kk = k + 32 * u;
                const bool in = kk + kq < K;  // K % 8 == 0: a chunk of 8 is in or out
                fa[u] = make_uint4(0, 0, 0, 0);
                if (in && live) fa[u] = *reinterpret_cast<const uint4*>(ap + kk);
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    fb[u][g] = make_uint4(0, 0, 0, 0);
                    if (in) fb[u][g] = *reinterpret_cast<const uint4*>(wp + g * gate_stride + kk);
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    if constexpr (__is_same(T, bf16))
                        acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(V, fa[u]), __builtin_bit_cast(V, fb[u][g]), acc[g], 0, 0, 0);
                    else
                        acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(V, fa[u]), __builtin_bit_cast(V, fb[u][g]), acc[g], 0, 0, 0);
                }
        }
    } else {
        const int r0 = row0 + 4 * (lane >> 4);
        const T* wp = W + (long long)(col0 + (lane & 15)) * K;
        for (int k = 0; k < K; k += 4) {  // K % 4 == 0
            float4 a[4], w[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                a[r] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (r0 + r < rows) a[r] = *reinterpret_cast<const float4*>(A + (long long)(r0 + r) * lda + k);
            }
#pragma unroll
            for (int g = 0; g < 4; ++g) w[g] = *reinterpret_cast<const float4*>(wp + g * gate_stride + k);
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float s = acc[g][r];
                    s = fmaf(a[r].x, w[g].x, s);
                    s = fmaf(a[r].y, w[g].y, s);
                    s = fmaf(a[r].z, w[g].z, s);
                    s = fmaf(a[r].w, w[g].w, s);
                    acc[g][r] = s;
                }
        }
    }
}

template <typename T>
__global__ __launch_bounds__(64) void lstm_fwd_step_kernel(LstmFwdArgs a) {
    const int lane = threadIdx.x & 63, H = a.H;
    const int col0 = blockIdx.x * 16, row0 = blockIdx.y * 16;
    lstm_f32x4 acc[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) acc[g] = lstm_f32x4{0.f, 0.f, 0.f, 0.f};
    if (a.hprev)
        tile_gates<T>(reinterpret_cast<const T*>(a.hprev), a.hprev_ld, a.B, row0, reinterpret_cast<const T*>(a.whh), H,
                      (long long)H * H, col0, acc);
    const int j = col0 + (lane & 15);
    const T* gx = reinterpret_cast<const T*>(a.gx);
    const T* bhh = reinterpret_cast<const T*>(a.bhh);
    float b[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) b[g] = to_f32(bhh[g * H + j]);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long long row = row0 + 4 * (lane >> 4) + r;
        if (row >= a.B) continue;
        float pre[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) pre[g] = acc[g][r] + b[g] + to_f32(gx[row * a.gx_ldb + g * H + j]);
        // the gates as they are stored: backward reads exactly these
        const T gi = from_f32<T>(sigmoid_f<T>(pre[0])), gf = from_f32<T>(sigmoid_f<T>(pre[1]));
        const T gg = from_f32<T>(tanhf(pre[2])), go = from_f32<T>(sigmoid_f<T>(pre[3]));
        const float cp = a.cprev ? to_f32(reinterpret_cast<const T*>(a.cprev)[row * a.cprev_ld + j]) : 0.f;
        const T c = from_f32<T>(fmaf(to_f32(gf), cp, to_f32(gi) * to_f32(gg)));
        const T h = from_f32<T>(to_f32(go) * tanhf(to_f32(c)));
        T* gates = reinterpret_cast<T*>(a.gates) + row * 4 * a.out_ld;
        gates[j] = gi;
        gates[H + j] = gf;
        gates[2 * H + j] = gg;
        gates[3 * H + j] = go;
        reinterpret_cast<T*>(a.c)[row * a.out_ld + j] = c;
        reinterpret_cast<T*>(a.y)[row * a.out_ld + j] = h;
        if (a.hT) reinterpret_cast<T*>(a.hT)[row * H + j] = h;
        if (a.cT) reinterpret_cast<T*>(a.cT)[row * H + j] = c;
    }
}

template <typename T>
__global__ __launch_bounds__(64) void lstm_bwd_step_kernel(LstmBwdArgs a) {
    const int lane = threadIdx.x & 63, H = a.H;
    const int col0 = blockIdx.x * 16, row0 = blockIdx.y * 16;
    lstm_f32x4 acc[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) acc[g] = lstm_f32x4{0.f, 0.f, 0.f, 0.f};
    // dG_{t+1} [B][4H] (rows 4 ld apart) times W_hh^T [H][4H]: one "gate" of width 4H, only acc[0] is used below
    if (a.dg_next) {
        const int lane16 = lane & 15;
        if constexpr (sizeof(T) == 2) {
            const int ar = row0 + lane16, kq = 8 * (lane >> 4), K = 4 * H;
            const bool live = ar < a.B;
            const T* ap = reinterpret_cast<const T*>(a.dg_next) + (long long)ar * 4 * a.ld + kq;
            const T* wp = reinterpret_cast<const T*>(a.whhT) + (long long)(col0 + lane16) * K + kq;
            constexpr int U = 4;  // (H % 16 == 0 gives 4H % 64 == 0: no partial k-step, but not always a whole pass)
            typedef typename H16<T>::vec V;
            for (int k = 0; k < K; k += 32 * U) {
                uint4 fa[U], fb[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int kk = k + 32 * u;
                    fa[u] = fb[u] = make_uint4(0, 0, 0, 0);
                    if (kk < K && live) fa[u] = *reinterpret_cast<const uint4*>(ap + kk);
                    if (kk < K) fb[u] = *reinterpret_cast<const uint4*>(wp + kk);
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if constexpr (__is_same(T, bf16))
                        acc[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(V, fa[u]), __builtin_bit_cast(V, fb[u]), acc[0], 0, 0, 0);
                    else
                        acc[0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(V, fa[u]), __builtin_bit_cast(V, fb[u]), acc[0], 0, 0, 0);
                }
            }
        } else {
            const int r0 = row0 + 4 * (lane >> 4), K = 4 * H;
            const T* A = reinterpret_cast<const T*>(a.dg_next);
            const T* wp = reinterpret_cast<const T*>(a.whhT) + (long long)(col0 + lane16) * K;
            for (int k = 0; k < K; k += 4) {
                const float4 w = *reinterpret_cast<const float4*>(wp + k);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (r0 + r >= a.B) continue;
                    const float4 v = *reinterpret_cast<const float4*>(A + (long long)(r0 + r) * 4 * a.ld + k);
                    float s = acc[0][r];
                    s = fmaf(v.x, w.x, s);
                    s = fmaf(v.y, w.y, s);
                    s = fmaf(v.z, w.z, s);
                    s = fmaf(v.w, w.w, s);
                    acc[0][r] = s;
                }
            }
        }
    }
    const int j = col0 + (lane & 15);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long long row = row0 + 4 * (lane >> 4) + r;
        if (row >= a.B) continue;
        const float dh = acc[0][r] + to_f32(reinterpret_cast<const T*>(a.dy)[row * a.ld + j]);
        const T* gates = reinterpret_cast<const T*>(a.gates) + row * 4 * a.ld;
        const float gi = to_f32(gates[j]), gf = to_f32(gates[H + j]), gg = to_f32(gates[2 * H + j]), go = to_f32(gates[3 * H + j]);
        const float tc = tanhf(to_f32(reinterpret_cast<const T*>(a.c)[row * a.ld + j]));
        const float cp = a.cprev ? to_f32(reinterpret_cast<const T*>(a.cprev)[row * a.cprev_ld + j]) : 0.f;
        const float carry = a.first ? 0.f : a.dc[row * H + j];
        const float dc = fmaf(dh * go, 1.f - tc * tc, carry);
        T* dg = reinterpret_cast<T*>(a.dg) + row * 4 * a.ld;
        dg[j] = from_f32<T>(dc * gg * gi * (1.f - gi));
        dg[H + j] = from_f32<T>(dc * cp * gf * (1.f - gf));
        dg[2 * H + j] = from_f32<T>(dc * gi * (1.f - gg * gg));
        dg[3 * H + j] = from_f32<T>(dh * tc * go * (1.f - go));
        a.dc[row * H + j] = dc * gf;
    }
}

// out [C][R] = in [R][C]^T
template <typename T>
__global__ __launch_bounds__(256) void lstm_transpose_kernel(const T* __restrict__ in, T* __restrict__ out, int R, int C) {
    __shared__ T tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
    for (int i = ty; i < 32; i += 8)
        if (r0 + i < R && c0 + tx < C) tile[i][tx] = in[(long long)(r0 + i) * C + c0 + tx];
    __syncthreads();
    for (int i = ty; i < 32; i += 8)
        if (c0 + i < C && r0 + tx < R) out[(long long)(c0 + i) * R + r0 + tx] = tile[tx][i];
}

inline size_t elem_size(int dtype) { return dtype == PK_F32 ? 4 : 2; }

}  // namespace

extern "C" size_t pk_lstm_bwd_scratch(long long B, int H, int dtype) {
    if (B < 1 || H < 1 || (dtype != PK_F32 && dtype != PK_BF16 && dtype != PK_F16)) return 0;
    Carve c{nullptr};
    c.take((size_t)B * H * 4);
    c.take((size_t)4 * H * H * elem_size(dtype));
    return c.total;
}

#define PK_LSTM_SHAPE_CHECKS(who)                                                                                       \
    PK_CHECK_ARG(B >= 1 && T >= 1 && H >= 1, who ": bad sizes (B=%lld T=%lld H=%d)", B, T, H);                            \
    PK_CHECK_ARG(dtype == PK_F32 || dtype == PK_BF16 || dtype == PK_F16, who ": dtype %d not supported", dtype);        \
    PK_CHECK_ARG(H % 16 == 0, who ": hidden size %d must be a multiple of 16", H);                                      \
    PK_CHECK_ARG((B + 15) / 16 <= 65535, who ": too many rows (B=%lld)", B);                                            \
    PK_CHECK_ARG(B * T * 4 * H < (1LL << 40), who ": sizes overflow (B=%lld T=%lld H=%d)", B, T, H)

extern "C" int pk_lstm_fwd(const void* gx, long long gx_ldb, long long gx_ldt, const void* w_hh, const void* b_hh,
                           const void* h0, const void* c0, void* y, void* c, void* gates, void* hT, void* cT, long long B,
                           long long T, int H, int dtype, void* stream) {
    PK_CHECK_ARG(gx && w_hh && b_hh && y && c && gates, "pk_lstm_fwd: null argument");
    PK_CHECK_ARG((h0 == nullptr) == (c0 == nullptr), "pk_lstm_fwd: h0 and c0 come together or not at all");
    PK_LSTM_SHAPE_CHECKS("pk_lstm_fwd");
    PK_CHECK_ARG(gx_ldt >= 4LL * H && gx_ldb >= 4LL * H && gx_ldt % 8 == 0 && gx_ldb % 8 == 0,
                 "pk_lstm_fwd: gx strides (%lld, %lld) must be multiples of 8 and at least 4H", gx_ldb, gx_ldt);
    PK_CHECK_ARG((((uintptr_t)w_hh | (uintptr_t)y | (uintptr_t)h0) % 16) == 0, "pk_lstm_fwd: w_hh, y and h0 must be 16-byte aligned");
    const size_t es = elem_size(dtype);
    const dim3 grid((unsigned)(H / 16), (unsigned)((B + 15) / 16));
    for (long long t = 0; t < T; ++t) {
        LstmFwdArgs a;
        a.gx = (const char*)gx + t * gx_ldt * es;
        a.whh = w_hh;
        a.bhh = b_hh;
        a.hprev = t ? (const char*)y + (t - 1) * H * es : h0;
        a.cprev = t ? (const char*)c + (t - 1) * H * es : c0;
        a.hprev_ld = a.cprev_ld = t ? T * H : H;
        a.y = (char*)y + t * H * es;
        a.c = (char*)c + t * H * es;
        a.gates = (char*)gates + t * 4 * H * es;
        a.hT = t == T - 1 ? hT : nullptr;
        a.cT = t == T - 1 ? cT : nullptr;
        a.gx_ldb = gx_ldb;
        a.out_ld = T * H;
        a.B = (int)B;
        a.H = H;
        PK_DTYPE_SWITCH(dtype, "pk_lstm_fwd", hipLaunchKernelGGL((lstm_fwd_step_kernel<T>), grid, dim3(64), 0, (hipStream_t)stream, a);)
        PK_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int pk_lstm_bwd(const void* dy, const void* w_hh, const void* y, const void* c, const void* gates, const void* c0,
                           void* dgates, long long B, long long T, int H, int dtype, void* scratch, size_t scratch_bytes,
                           void* stream) {
    (void)y;
    PK_CHECK_ARG(dy && w_hh && c && gates && dgates, "pk_lstm_bwd: null argument");
    PK_LSTM_SHAPE_CHECKS("pk_lstm_bwd");
    const size_t need = pk_lstm_bwd_scratch(B, H, dtype);
    PK_CHECK_ARG(scratch && scratch_bytes >= need, "pk_lstm_bwd: scratch too small (%zu < %zu)", scratch ? scratch_bytes : (size_t)0, need);
    PK_CHECK_ARG((((uintptr_t)w_hh | (uintptr_t)dgates | (uintptr_t)scratch) % 16) == 0, "pk_lstm_bwd: w_hh, dgates and scratch must be 16-byte aligned");
    const size_t es = elem_size(dtype);
    Carve cv{(char*)scratch};
    float* dc = cv.take<float>((size_t)B * H * 4);
    void* whhT = cv.take((size_t)4 * H * H * es);
    hipStream_t st = (hipStream_t)stream;
    if (T > 1) {  // W_hh [4H][H] -> [H][4H]
        const dim3 tg((unsigned)((H + 31) / 32), (unsigned)((4 * H + 31) / 32));
        PK_DTYPE_SWITCH(dtype, "pk_lstm_bwd", hipLaunchKernelGGL((lstm_transpose_kernel<T>), tg, dim3(256), 0, st, (const T*)w_hh, (T*)whhT, 4 * H, H);)
        PK_LAUNCH_CHECK();
    }
    const dim3 grid((unsigned)(H / 16), (unsigned)((B + 15) / 16));
    for (long long t = T - 1; t >= 0; --t) {
        LstmBwdArgs a;
        a.dy = (const char*)dy + t * H * es;
        a.dg_next = t == T - 1 ? nullptr : (const char*)dgates + (t + 1) * 4 * H * es;
        a.whhT = whhT;
        a.gates = (const char*)gates + t * 4 * H * es;
        a.c = (const char*)c + t * H * es;
        a.cprev = t ? (const char*)c + (t - 1) * H * es : c0;
        a.cprev_ld = t ? T * H : H;
        a.dg = (char*)dgates + t * 4 * H * es;
        a.dc = dc;
        a.ld = T * H;
        a.B = (int)B;
        a.H = H;
        a.first = t == T - 1;
        PK_DTYPE_SWITCH(dtype, "pk_lstm_bwd", hipLaunchKernelGGL((lstm_bwd_step_kernel<T>), grid, dim3(64), 0, st, a);)
        PK_LAUNCH_CHECK();
    }
    return 0;
}
