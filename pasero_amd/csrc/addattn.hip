// Additive (Bahdanau) single-head attention of `hybrid_transformer`'s decoder (pasero/models/hybrid.py AttentionLayer):
//     score[b,t,s] = sum_h w[h] tanh(k[b,s,h] + q[b,t,h])      q, k: the projections' outputs, biases included
//     p = softmax_s(score masked to -inf at padded keys)        ctx[b,t,:] = sum_s p[b,t,s] value[b,s,:]
// The per-op form materialises (B, T, S, H) for the tanh; here one workgroup owns AA_TQ queries of one sentence, walks the
// keys and keeps only scores (fp32, LDS).  inner_proj's bias shifts a row's scores equally and is left out.
//
// pk_addattn_fwd, per workgroup of 4 waves (each wave owns 2 of the 8 queries):
//   1. q rows and w to LDS as fp32;  2. lanes walk the keys 64 at a time, 16-byte chunks of k[s, :] against the LDS rows
//   (a chunk serves both queries of the wave);  3. softmax per query in fp32 (wave butterflies), probabilities rounded to the
//   storage type — masked keys exactly 0 — written out and kept in LDS;  4. ctx from the ROUNDED probabilities (what
//   backward reads), lanes across D.
// pk_addattn_bwd, deterministic, no atomics:
//   pass 1 (same query tiling): dp = dctx value^T, ds = p (dp - sum_s p dp) -> fp32 scratch [B][T][S]; dq = sum_s e with
//     e = ds w (1 - tanh^2) recomputed, lanes across H; the workgroup's share of dw = sum ds tanh, waves added in order, to
//     a partial row per workgroup;
//   pass 2 (8 keys of one sentence per workgroup, 2 per wave): dk = sum_t e (tanh recomputed) and dvalue = p^T dctx;
//   pass 3: dw = the partial rows added in a fixed tree (a wave per h: strided rows per lane, then the butterfly).
// Keys with ds == 0 for both queries of a wave (every padded key) are skipped.
// The score / context products are plain fp32 multiply-adds for every dtype: the kernel's time is the B T S H tanh evaluations
// (one v_exp_f32 + one v_rcp_f32 each for the 16-bit types, tanhf for fp32), next to which p value is 2 D / (~10 H) of the work.
#include "common.h"

namespace {

// LDS per workgroup: up to gfx950's 160 KiB (asked for per kernel with hipFuncSetAttribute).  The q / dctx rows of 8 queries
// and the scores live there: forward (9 H + 8 S) * 4 bytes, backward (13 H + 8 D + 8 S) * 4 — H = D = 1024 trains up to
// S = 2432, H = 2048 with D = 1024 up to S = 768.
constexpr int AA_TQ = 8, AA_QPW = 2, AA_LDS_MAX = 160 * 1024;

template <typename T> __device__ __forceinline__ float aa_tanh(float x) {
    if constexpr (sizeof(T) == 2) return 1.f - 2.f * pk_rcp(1.f + __expf(2.f * x));  // exp -> inf: 1; exp -> 0: -1
    else return tanhf(x);
}
template <typename T> __device__ __forceinline__ float aa_exp(float x) {
    if constexpr (sizeof(T) == 2) return __expf(x);
    else return expf(x);
}

// A running fp32 sum.  The fp32 model compensates it (Kahan): a chain of S or H plain additions loses up to that many half-ulps,
// visibly more than the blocked sums of a GEMM library over the same terms, and the fp32 path exists for parity.  For the
// 16-bit types the rounding of the output hides the difference and the sum is plain.
template <typename T> struct AaSum {
    float s = 0.f, c = 0.f;
    __device__ __forceinline__ void add(float x) {
        if constexpr (sizeof(T) == 4) {
            const float y = x - c, t = s + y;
            c = (t - s) - y;
            s = t;
        } else {
            s += x;
        }
    }
};

struct AaArgs {
    const void *q, *k, *w, *value, *probs_in, *dctx;
    const unsigned char* pad;
    void *probs, *ctx, *dq, *dk, *dw, *dvalue;
    float *ds, *dw_part;
    int B, T, S, H, D;
};

// rows t0 .. t0 + AA_TQ of src [.][n] (zeros past T) to dst [AA_TQ][n] as fp32
template <typename T>
__device__ __forceinline__ void aa_rows_to_lds(const T* src, float* dst, int t0, int Tn, int n) {
    for (int i = threadIdx.x; i < AA_TQ * n; i += 256) {
        const int r = i / n, c = i - r * n;
        dst[i] = t0 + r < Tn ? to_f32(src[(long long)(t0 + r) * n + c]) : 0.f;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void addattn_fwd_kernel(AaArgs a) {
    extern __shared__ float aa_smem[];
    const int H = a.H, S = a.S, D = a.D, Tn = a.T;
    float* qs = aa_smem;           // [AA_TQ][H]
    float* ws = qs + AA_TQ * H;    // [H]
    float* sc = ws + H;            // [AA_TQ][S]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y, t0 = blockIdx.x * AA_TQ;
    const T* q = reinterpret_cast<const T*>(a.q) + (long long)b * Tn * H;
    const T* k = reinterpret_cast<const T*>(a.k) + (long long)b * S * H;
    const T* value = reinterpret_cast<const T*>(a.value) + (long long)b * S * D;
    const unsigned char* pad = a.pad ? a.pad + (long long)b * S : nullptr;
    aa_rows_to_lds<T>(q, qs, t0, Tn, H);
    for (int i = tid; i < H; i += 256) ws[i] = to_f32(reinterpret_cast<const T*>(a.w)[i]);
    __syncthreads();

    const int q0 = wave * AA_QPW;
    const float* qa = qs + q0 * H;
    const float* qb = qa + H;
    // a wave whose two queries lie beyond T (3 of 4 waves at T = 1, a decoding step) has nothing to compute: it only keeps
    // the barriers.  (Wave-uniform, and there is no barrier inside what it skips.)
    const bool wave_live = t0 + q0 < Tn, two_live = t0 + q0 + 1 < Tn;
    for (int s = lane; wave_live && s < S; s += 64) {
        float s0 = -INFINITY, s1 = -INFINITY;
        if (!(pad && pad[s])) {
            AaSum<T> a0, a1;
            const T* kr = k + (long long)s * H;
            for (int h = 0; h < H; h += Vec16<T>::N) {
                const Vec16<T> kv = load16<T>(kr + h);
#pragma unroll
                for (int e = 0; e < Vec16<T>::N; ++e) {
                    const float kk = kv.get(e), wh = ws[h + e];
                    a0.add(wh * aa_tanh<T>(kk + qa[h + e]));
                    if (two_live) a1.add(wh * aa_tanh<T>(kk + qb[h + e]));
                }
            }
            s0 = a0.s;
            s1 = a1.s;
        }
        sc[q0 * S + s] = s0;
        sc[(q0 + 1) * S + s] = s1;
    }
    __syncthreads();

#pragma unroll
    for (int qi = 0; qi < AA_QPW; ++qi) {
        float* row = sc + (q0 + qi) * S;
        const int t = t0 + q0 + qi;
        if (t >= Tn) continue;  // (wave-uniform: all 64 lanes reach the butterflies below or none does)
        float m = -INFINITY;
        for (int s = lane; s < S; s += 64) m = fmaxf(m, row[s]);
        m = wave_max(m);
        AaSum<T> part;
        for (int s = lane; s < S; s += 64) {
            const float e = aa_exp<T>(row[s] - m);  // masked: exp(-inf) = 0 exactly
            row[s] = e;
            part.add(e);
        }
        const float sum = wave_sum(part.s);
        const float inv = 1.f / sum;
        T* pr = reinterpret_cast<T*>(a.probs) + ((long long)b * Tn + t) * S;
        for (int s = lane; s < S; s += 64) {
            const T p = from_f32<T>(row[s] * inv);
            row[s] = to_f32(p);
            if (t < Tn) pr[s] = p;
        }
    }
    __syncthreads();

#pragma unroll
    for (int qi = 0; qi < AA_QPW; ++qi) {
        const float* row = sc + (q0 + qi) * S;
        const int t = t0 + q0 + qi;
        if (t >= Tn) continue;
        T* out = reinterpret_cast<T*>(a.ctx) + ((long long)b * Tn + t) * D;
        for (int d = lane; d < D; d += 64) {
            AaSum<T> acc;
            for (int s = 0; s < S; ++s) acc.add(row[s] * to_f32(value[(long long)s * D + d]));
            out[d] = from_f32<T>(acc.s);
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void addattn_bwd_q_kernel(AaArgs a) {
    extern __shared__ float aa_smem[];
    const int H = a.H, S = a.S, D = a.D, Tn = a.T;
    float* qs = aa_smem;            // [AA_TQ][H]
    float* ws = qs + AA_TQ * H;     // [H]
    float* dcs = ws + H;            // [AA_TQ][D]
    float* dss = dcs + AA_TQ * D;   // [AA_TQ][S]
    float* dwp = dss + AA_TQ * S;   // [4][H]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y, t0 = blockIdx.x * AA_TQ;
    const T* q = reinterpret_cast<const T*>(a.q) + (long long)b * Tn * H;
    const T* k = reinterpret_cast<const T*>(a.k) + (long long)b * S * H;
    const T* value = reinterpret_cast<const T*>(a.value) + (long long)b * S * D;
    const T* dctx = reinterpret_cast<const T*>(a.dctx) + (long long)b * Tn * D;
    aa_rows_to_lds<T>(q, qs, t0, Tn, H);
    aa_rows_to_lds<T>(dctx, dcs, t0, Tn, D);
    for (int i = tid; i < H; i += 256) ws[i] = to_f32(reinterpret_cast<const T*>(a.w)[i]);
    __syncthreads();

    const int q0 = wave * AA_QPW;
    // dp and ds, lanes across the keys
    {
        const float* da = dcs + q0 * D;
        const float* db = da + D;
        const bool live0 = t0 + q0 < Tn, live1 = t0 + q0 + 1 < Tn;
        const T* pa = reinterpret_cast<const T*>(a.probs_in) + ((long long)b * Tn + t0 + q0) * S;
        const T* pb = pa + S;
        AaSum<T> del0, del1;
        for (int s = lane; live0 && s < S; s += 64) {  // (a wave without a live query skips: wave-uniform, no barrier inside)
            const T* vr = value + (long long)s * D;
            AaSum<T> d0, d1;
            for (int d = 0; d < D; d += Vec16<T>::N) {
                const Vec16<T> vv = load16<T>(vr + d);
#pragma unroll
                for (int e = 0; e < Vec16<T>::N; ++e) {
                    const float v = vv.get(e);
                    d0.add(da[d + e] * v);
                    d1.add(db[d + e] * v);
                }
            }
            dss[q0 * S + s] = d0.s;
            dss[(q0 + 1) * S + s] = d1.s;
            if (live0) del0.add(to_f32(pa[s]) * d0.s);
            if (live1) del1.add(to_f32(pb[s]) * d1.s);
        }
        const float sum0 = wave_sum(del0.s), sum1 = wave_sum(del1.s);
        float* ga = a.ds + ((long long)b * Tn + t0 + q0) * S;
        float* gb = ga + S;
        for (int s = lane; live0 && s < S; s += 64) {
            const float e0 = live0 ? to_f32(pa[s]) * (dss[q0 * S + s] - sum0) : 0.f;
            const float e1 = live1 ? to_f32(pb[s]) * (dss[(q0 + 1) * S + s] - sum1) : 0.f;
            dss[q0 * S + s] = e0;
            dss[(q0 + 1) * S + s] = e1;
            if (live0) ga[s] = e0;
            if (live1) gb[s] = e1;
        }
    }
    __syncthreads();

    // dq and this workgroup's share of dw, lanes across H
    {
        const float* ea = dss + q0 * S;
        const float* eb = ea + S;
        const bool wave_live = t0 + q0 < Tn;  // (a wave without one still writes its zero share of dw)
        for (int h = lane; h < H; h += 64) {
            const float wh = ws[h], qa = qs[q0 * H + h], qb = qs[(q0 + 1) * H + h];
            AaSum<T> dq0, dq1, dw;
            for (int s = 0; wave_live && s < S; ++s) {
                const float e0 = ea[s], e1 = eb[s];
                if (e0 == 0.f && e1 == 0.f) continue;  // (wave-uniform: the values come from LDS)
                const float kk = to_f32(k[(long long)s * H + h]);
                const float th0 = aa_tanh<T>(kk + qa), th1 = aa_tanh<T>(kk + qb);
                dq0.add(e0 * (1.f - th0 * th0));
                dq1.add(e1 * (1.f - th1 * th1));
                dw.add(e0 * th0);
                dw.add(e1 * th1);
            }
            if (t0 + q0 < Tn) reinterpret_cast<T*>(a.dq)[((long long)b * Tn + t0 + q0) * H + h] = from_f32<T>(dq0.s * wh);
            if (t0 + q0 + 1 < Tn) reinterpret_cast<T*>(a.dq)[((long long)b * Tn + t0 + q0 + 1) * H + h] = from_f32<T>(dq1.s * wh);
            dwp[wave * H + h] = dw.s;
        }
    }
    __syncthreads();
    float* part = a.dw_part + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * H;
    for (int h = tid; h < H; h += 256) part[h] = ((dwp[h] + dwp[H + h]) + dwp[2 * H + h]) + dwp[3 * H + h];
}

template <typename T>
__global__ __launch_bounds__(256) void addattn_bwd_k_kernel(AaArgs a) {
    const int H = a.H, S = a.S, D = a.D, Tn = a.T;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.y, s0 = blockIdx.x * AA_TQ + wave * AA_QPW;
    if (s0 >= S) return;  // (wave-uniform; no barrier below)
    const bool two = s0 + 1 < S;
    const int s1 = two ? s0 + 1 : s0;
    const T* q = reinterpret_cast<const T*>(a.q) + (long long)b * Tn * H;
    const T* k = reinterpret_cast<const T*>(a.k) + (long long)b * S * H;
    const T* dctx = reinterpret_cast<const T*>(a.dctx) + (long long)b * Tn * D;
    const T* probs = reinterpret_cast<const T*>(a.probs_in) + (long long)b * Tn * S;
    const float* ds = a.ds + (long long)b * Tn * S;
    const T* w = reinterpret_cast<const T*>(a.w);
    T* dk = reinterpret_cast<T*>(a.dk) + (long long)b * S * H;
    T* dv = reinterpret_cast<T*>(a.dvalue) + (long long)b * S * D;
    for (int h = lane; h < H; h += 64) {
        const float wh = to_f32(w[h]), k0 = to_f32(k[(long long)s0 * H + h]), k1 = to_f32(k[(long long)s1 * H + h]);
        AaSum<T> a0, a1;
        for (int t = 0; t < Tn; ++t) {
            const float e0 = ds[(long long)t * S + s0], e1 = ds[(long long)t * S + s1];
            if (e0 == 0.f && e1 == 0.f) continue;  // (wave-uniform addresses)
            const float qv = to_f32(q[(long long)t * H + h]);
            const float th0 = aa_tanh<T>(k0 + qv), th1 = aa_tanh<T>(k1 + qv);
            a0.add(e0 * (1.f - th0 * th0));
            a1.add(e1 * (1.f - th1 * th1));
        }
        dk[(long long)s0 * H + h] = from_f32<T>(a0.s * wh);
        if (two) dk[(long long)s1 * H + h] = from_f32<T>(a1.s * wh);
    }
    for (int d = lane; d < D; d += 64) {
        AaSum<T> a0, a1;
        for (int t = 0; t < Tn; ++t) {
            const float g = to_f32(dctx[(long long)t * D + d]);
            a0.add(to_f32(probs[(long long)t * S + s0]) * g);
            a1.add(to_f32(probs[(long long)t * S + s1]) * g);
        }
        dv[(long long)s0 * D + d] = from_f32<T>(a0.s);
        if (two) dv[(long long)s1 * D + d] = from_f32<T>(a1.s);
    }
}

// dw[h] = the n partial rows added in a fixed tree: one wave per h, lane l adds rows l, l + 64, ... in order, then the wave
// butterfly — the same bits on every run, a chain of n / 64 + 6 additions instead of n
template <typename T>
__global__ __launch_bounds__(256) void addattn_dw_kernel(const float* __restrict__ part, T* __restrict__ dw, long long n, int H) {
    const int lane = threadIdx.x & 63, h = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (h >= H) return;  // (wave-uniform)
    AaSum<T> s;
    for (long long i = lane; i < n; i += 64) s.add(part[i * H + h]);
    const float total = wave_sum(s.s);
    if (lane == 0) dw[h] = from_f32<T>(total);
}

template <typename K> int aa_allow_lds(K kernel, const char* who) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, AA_LDS_MAX);
    if (e != hipSuccess) {
        pk_set_error("%s: hipFuncSetAttribute: %s", who, hipGetErrorString(e));
        return (int)e;
    }
    return 0;
}

inline size_t fwd_lds(int S, int H) { return ((size_t)AA_TQ * H + H + (size_t)AA_TQ * S) * 4; }
inline size_t bwd_lds(int S, int H, int D) { return ((size_t)AA_TQ * H + H + (size_t)AA_TQ * D + (size_t)AA_TQ * S + 4 * (size_t)H) * 4; }

}  // namespace

#define PK_ADDATTN_SHAPE_CHECKS(who)                                                                                       \
    PK_CHECK_ARG(B >= 1 && T >= 1 && S >= 1 && H >= 1 && D >= 1, who ": bad sizes (B=%d T=%d S=%d H=%d D=%d)", B, T, S, H, D); \
    PK_CHECK_ARG(dtype == PK_F32 || dtype == PK_BF16 || dtype == PK_F16, who ": dtype %d not supported", dtype);           \
    PK_CHECK_ARG(H % 16 == 0, who ": hidden size %d must be a multiple of 16", H);                                         \
    PK_CHECK_ARG(D % 8 == 0, who ": value width %d must be a multiple of 8", D);                                           \
    PK_CHECK_ARG(B <= 65535, who ": too many sentences (B=%d)", B)

extern "C" size_t pk_addattn_bwd_scratch(int B, int T, int S, int H) {
    if (B < 1 || T < 1 || S < 1 || H < 1) return 0;
    Carve c{nullptr};
    c.take((size_t)B * T * S * 4);
    c.take((size_t)B * ((T + AA_TQ - 1) / AA_TQ) * H * 4);
    return c.total;
}

extern "C" int pk_addattn_fwd(const void* q, const void* k, const void* w, const unsigned char* key_pad, const void* value,
                              void* probs, void* ctx, int B, int T, int S, int H, int D, int dtype, void* stream) {
    PK_CHECK_ARG(q && k && w && value && probs && ctx, "pk_addattn_fwd: null argument");
    PK_ADDATTN_SHAPE_CHECKS("pk_addattn_fwd");
    PK_CHECK_ARG((((uintptr_t)k | (uintptr_t)value) % 16) == 0, "pk_addattn_fwd: k and value must be 16-byte aligned");
    const size_t lds = fwd_lds(S, H);
    PK_CHECK_ARG(lds <= (size_t)AA_LDS_MAX, "pk_addattn_fwd: S=%d with H=%d needs %zu bytes of LDS, the limit is %d", S, H, lds, AA_LDS_MAX);
    AaArgs a{};
    a.q = q, a.k = k, a.w = w, a.value = value, a.pad = key_pad, a.probs = probs, a.ctx = ctx;
    a.B = B, a.T = T, a.S = S, a.H = H, a.D = D;
    const dim3 grid((unsigned)((T + AA_TQ - 1) / AA_TQ), (unsigned)B);
    PK_DTYPE_SWITCH(dtype, "pk_addattn_fwd",
        static const int attr = aa_allow_lds(&addattn_fwd_kernel<T>, "pk_addattn_fwd");
        if (attr != 0) return attr;
        hipLaunchKernelGGL((addattn_fwd_kernel<T>), grid, dim3(256), lds, (hipStream_t)stream, a);)
    PK_LAUNCH_CHECK();
    return 0;
}

extern "C" int pk_addattn_bwd(const void* dctx, const void* q, const void* k, const void* w, const void* value,
                              const void* probs, void* dq, void* dk, void* dw, void* dvalue, int B, int T, int S, int H, int D,
                              int dtype, void* scratch, size_t scratch_bytes, void* stream) {
    PK_CHECK_ARG(dctx && q && k && w && value && probs && dq && dk && dw && dvalue, "pk_addattn_bwd: null argument");
    PK_ADDATTN_SHAPE_CHECKS("pk_addattn_bwd");
    PK_CHECK_ARG((((uintptr_t)k | (uintptr_t)value) % 16) == 0, "pk_addattn_bwd: k and value must be 16-byte aligned");
    const size_t lds = bwd_lds(S, H, D);
    PK_CHECK_ARG(lds <= (size_t)AA_LDS_MAX, "pk_addattn_bwd: S=%d with H=%d, D=%d needs %zu bytes of LDS, the limit is %d", S, H, D, lds, AA_LDS_MAX);
    const size_t need = pk_addattn_bwd_scratch(B, T, S, H);
    PK_CHECK_ARG(scratch && scratch_bytes >= need, "pk_addattn_bwd: scratch too small (%zu < %zu)", scratch ? scratch_bytes : (size_t)0, need);
    const int qt = (T + AA_TQ - 1) / AA_TQ;
    Carve c{(char*)scratch};
    AaArgs a{};
    a.ds = c.take<float>((size_t)B * T * S * 4);
    a.dw_part = c.take<float>((size_t)B * qt * H * 4);
    a.q = q, a.k = k, a.w = w, a.value = value, a.probs_in = probs, a.dctx = dctx;
    a.dq = dq, a.dk = dk, a.dw = dw, a.dvalue = dvalue;
    a.B = B, a.T = T, a.S = S, a.H = H, a.D = D;
    hipStream_t st = (hipStream_t)stream;
    const dim3 gq((unsigned)qt, (unsigned)B), gk((unsigned)((S + AA_TQ - 1) / AA_TQ), (unsigned)B);
    PK_DTYPE_SWITCH(dtype, "pk_addattn_bwd",
        static const int attr = aa_allow_lds(&addattn_bwd_q_kernel<T>, "pk_addattn_bwd");
        if (attr != 0) return attr;
        hipLaunchKernelGGL((addattn_bwd_q_kernel<T>), gq, dim3(256), lds, st, a);
        hipLaunchKernelGGL((addattn_bwd_k_kernel<T>), gk, dim3(256), 0, st, a);
        hipLaunchKernelGGL((addattn_dw_kernel<T>), dim3((unsigned)((H + 3) / 4)), dim3(256), 0, st, a.dw_part, (T*)dw, (long long)B * qt, H);)
    PK_LAUNCH_CHECK();
    return 0;
}
