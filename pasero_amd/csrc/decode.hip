// One incremental decoding step (one new token per sentence) of the Transformer decoder stack, driven from native code:
// the ~75 kernel launches of a step are issued by one C call instead of ~90 Python-level op dispatches (measured: the
// Python path costs 2.05 ms per step at any batch size — pure launch overhead).
//
// Replaces, for T = 1 and a non-empty incremental state: TransformerDecoder.forward (pasero/models/transformer.py:831-898),
// TransformerDecoderLayer.forward/.self_attention/.cross_attention/.ffn (:1341-1417, :1246-1320, :1224-1244) and the
// KV-cache branch of MultiheadAttention.forward (pasero/models/modules.py:621-641).  Differences by design:
//   * the self-attention K/V cache is a preallocated [B][cap][D] buffer per layer that the new row is appended to
//     (the reference re-concatenates the whole cache every step, modules.py:636-637);
//   * the cross-attention K/V projections of the encoder output are computed once per sentence and passed in
//     (the reference recomputes k_proj/v_proj(encoder_out) every step, modules.py:612-615).
// Every matrix product, LayerNorm and attention call is the same pk_* kernel the training path uses.
#include <utility>
#include "common.h"

namespace {

// append this step's K and V rows (columns [D, 3D) of the packed projection) to the per-layer caches at position t
template <typename T>
__global__ __launch_bounds__(256) void kv_append_kernel(const T* __restrict__ qkv, T* __restrict__ ck,
                                                        T* __restrict__ cv, int d, int t, long long cap) {
    constexpr int EPV = 16 / sizeof(T);
    const int b = blockIdx.x;
    const T* src = qkv + (long long)b * 3 * d + d;
    T* dk = ck + ((long long)b * cap + t) * d;
    T* dv = cv + ((long long)b * cap + t) * d;
    for (int c = threadIdx.x * EPV; c < d; c += blockDim.x * EPV) {
        store16<T>(dk + c, load16<T>(src + c));
        store16<T>(dv + c, load16<T>(src + d + c));
    }
}

// greedy choice: first index of the row maximum (torch.argmax semantics on ties: lowest index)
template <typename T>
__global__ __launch_bounds__(256) void argmax_rows_kernel(const T* __restrict__ x, long long ld, long long n,
                                                          long long* __restrict__ out, long long out_stride) {
    const long long row = blockIdx.x;
    const T* p = x + row * ld;
    float best = -INFINITY;
    long long bi = n;
    for (long long i = threadIdx.x; i < n; i += blockDim.x) {
        float v = to_f32(p[i]);
        if (v > best || (v == best && i < bi)) { best = v; bi = i; }
    }
    __shared__ float sv[256];
    __shared__ long long si[256];
    sv[threadIdx.x] = best;
    si[threadIdx.x] = bi;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            float v = sv[threadIdx.x + s];
            long long i = si[threadIdx.x + s];
            if (v > sv[threadIdx.x] || (v == sv[threadIdx.x] && i < si[threadIdx.x])) { sv[threadIdx.x] = v; si[threadIdx.x] = i; }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) out[row * out_stride] = si[0] < n ? si[0] : 0;
}

struct Scratch {
    char *x0, *x1, *h, *qkv, *q, *o, *ff, *ad, *moe;
    float *lse, *mean, *rstd;
    size_t total, ad_bytes, moe_bytes;
};
// `adapters` adds, behind everything else, the largest three-launch scratch one of them needs; `moe`, behind that, the
// largest pk_moerows scratch among the layers
Scratch carve(const PkDecoderPlan* p, int B, char* base, const PkAdapterStack* adapters, const PkMoeLayer* moe) {
    const size_t es = p->dtype == PK_F32 ? 4 : 2;
    Scratch s;
    Carve c{base};
    s.x0 = c.take((size_t)B * p->d * es);
    s.x1 = c.take((size_t)B * p->d * es);
    s.h = c.take((size_t)B * p->d * es);
    s.qkv = c.take((size_t)B * 3 * p->d * es);
    s.q = c.take((size_t)B * p->d * es);
    s.o = c.take((size_t)B * p->d * es);
    s.ff = c.take((size_t)B * p->ffn * es);
    s.lse = c.take<float>((size_t)B * p->heads * 4);
    s.mean = c.take<float>((size_t)B * 4);
    s.rstd = c.take<float>((size_t)B * 4);
    s.ad_bytes = 0;
    for (int l = 0; adapters && l < p->n_layers; ++l)
        for (int i = 0; i < adapters[l].n && i < PK_ADAPTER_STACK_MAX; ++i) {
            const size_t need = pk_adapter_rows_step_scratch(B, p->d, adapters[l].a[i].p, p->dtype);
            if (need > s.ad_bytes) s.ad_bytes = need;
        }
    s.ad = c.take(s.ad_bytes);
    s.moe_bytes = 0;
    for (int l = 0; moe && l < p->n_layers; ++l)
        if (moe[l].E > 0) {
            const size_t need = pk_moerows_scratch(B, moe[l].E, p->d, moe[l].F, p->dtype);
            if (need > s.moe_bytes) s.moe_bytes = need;
        }
    s.moe = c.take(s.moe_bytes);
    s.total = c.total;
    return s;
}

}  // namespace

extern "C" size_t pk_decoder_step_scratch_moe(const PkDecoderPlan* plan, int B, const PkAdapterStack* adapters,
                                              const PkMoeLayer* moe) {
    return carve(plan, B > 0 ? B : 1, nullptr, adapters, moe).total;
}
extern "C" size_t pk_decoder_step_scratch_ex(const PkDecoderPlan* plan, int B, const PkAdapterStack* adapters) {
    return pk_decoder_step_scratch_moe(plan, B, adapters, nullptr);
}
extern "C" size_t pk_decoder_step_scratch(const PkDecoderPlan* plan, int B) {
    return pk_decoder_step_scratch_ex(plan, B, nullptr);
}

#define RC(call)                 \
    do {                         \
        int rc_ = (call);        \
        if (rc_ != 0) return rc_; \
    } while (0)

extern "C" int pk_decoder_step_moe(const PkDecoderPlan* plan, const long long* ids, int B, int t, int pos_start,
                                   void* const* self_k, void* const* self_v, long long cap, const void* const* cross_kv,
                                   const unsigned char* enc_mask, int S, void* scratch, size_t scratch_bytes, void* logits,
                                   long long ld_logits, const PkAdapterStack* adapters, const PkMoeLayer* moe, void* stream) {
    PK_CHECK_ARG(plan && ids && self_k && self_v && cross_kv && scratch && logits, "pk_decoder_step: null argument");
    PK_CHECK_ARG(B > 0 && t >= 0 && t < cap && S > 0, "pk_decoder_step: bad sizes (B=%d t=%d cap=%lld S=%d)", B, t, cap, S);
    PK_CHECK_ARG(plan->d % 64 == 0 && plan->heads * 64 == plan->d, "pk_decoder_step: head_dim must be 64");
    PK_CHECK_ARG(plan->dtype == PK_F32 || plan->dtype == PK_BF16 || plan->dtype == PK_F16, "pk_decoder_step: bad dtype");
    for (int l = 0; adapters && l < plan->n_layers; ++l) {
        PK_CHECK_ARG(adapters[l].n >= 0 && adapters[l].n <= PK_ADAPTER_STACK_MAX, "pk_decoder_step: layer %d has %d adapters (0..%d)",
                     l, adapters[l].n, PK_ADAPTER_STACK_MAX);
        for (int i = 0; i < adapters[l].n; ++i)
            PK_CHECK_ARG(adapters[l].a[i].down_w && adapters[l].a[i].up_w && adapters[l].a[i].p > 0,
                         "pk_decoder_step: adapter %d of layer %d is incomplete", i, l);
    }
    for (int l = 0; moe && l < plan->n_layers; ++l) {
        if (moe[l].E == 0) continue;
        PK_CHECK_ARG(moe[l].gate_w && moe[l].w1 && moe[l].w2, "pk_decoder_step: mixture of layer %d is incomplete", l);
        PK_CHECK_ARG(pk_moerows_scratch(B, moe[l].E, plan->d, moe[l].F, plan->dtype) > 0,
                     "pk_decoder_step: mixture of layer %d: E = %d, F = %d are not sizes pk_moerows takes", l, moe[l].E, moe[l].F);
    }
    Scratch s = carve(plan, B, (char*)scratch, adapters, moe);
    PK_CHECK_ARG(scratch_bytes >= s.total, "pk_decoder_step: scratch too small (%zu < %zu)", scratch_bytes, s.total);
    const int D = plan->d, H = plan->heads, F = plan->ffn, dt = plan->dtype;
    const float scale = plan->scaled_attn ? 0.125f : 1.f;
    hipStream_t st = (hipStream_t)stream;
    char *x = s.x0, *xn = s.x1;

    // residual + LayerNorm of a sub-block: post-norm  x <- LN(y + x);  pre-norm  x <- y + x (no LN here)
    auto block_end = [&](const void* y, const void* g, const void* b) -> int {
        if (plan->prenorm) RC(pk_residual_ln_fwd(y, x, nullptr, nullptr, xn, nullptr, nullptr, nullptr, B, D, plan->eps, 0.f, 0, 0, dt, stream));
        else RC(pk_residual_ln_fwd(y, x, g, b, nullptr, xn, s.mean, s.rstd, B, D, plan->eps, 0.f, 0, 0, dt, stream));
        std::swap(x, xn);
        return 0;
    };
    // input of a sub-block: pre-norm LN(x) -> h, post-norm x itself
    auto block_in = [&](const void* g, const void* b, const char** in) -> int {
        if (!plan->prenorm) { *in = x; return 0; }
        RC(pk_residual_ln_fwd(x, nullptr, g, b, nullptr, s.h, s.mean, s.rstd, B, D, plan->eps, 0.f, 0, 0, dt, stream));
        *in = s.h;
        return 0;
    };
    auto linear = [&](const void* in, const void* w, const void* b, void* out, int n, int k, int act) -> int {
        return pk_gemm(in, w, out, b, nullptr, nullptr, B, n, k, k, k, n, 0, 0, 0, 0, act, 0, 1.f, dt, 1, nullptr, 0,
                       nullptr, stream);
    };

    // token + position embedding (transformer.py:866-878): one row per sentence, position = pos_start
    RC(pk_embed_fwd(ids, plan->embed, plan->pos, x, B, 1, D, plan->vocab, plan->embed_scale, pos_start, 0.f, 0, 0, dt,
                    stream));
    if (plan->embed_ln_g) {
        RC(pk_residual_ln_fwd(x, nullptr, plan->embed_ln_g, plan->embed_ln_b, nullptr, xn, s.mean, s.rstd, B, D, plan->eps,
                              0.f, 0, 0, dt, stream));
        std::swap(x, xn);
    }
    const size_t es = dt == PK_F32 ? 4 : 2;
    for (int l = 0; l < plan->n_layers; ++l) {
        const PkDecoderLayerWeights& w = plan->layers[l];
        const char* in;
        // ---- self-attention over the cache (keys 0..t) ----
        RC(block_in(w.ln1_g, w.ln1_b, &in));
        RC(linear(in, w.qkv_w, w.qkv_b, s.qkv, 3 * D, D, PK_ACT_NONE));
        if (dt != PK_F32)  // a 16-bit row copy: bf16 and fp16 alike
            hipLaunchKernelGGL((kv_append_kernel<bf16>), dim3(B), dim3(64), 0, st, (const bf16*)s.qkv, (bf16*)self_k[l],
                               (bf16*)self_v[l], D, t, cap);
        else
            hipLaunchKernelGGL((kv_append_kernel<float>), dim3(B), dim3(128), 0, st, (const float*)s.qkv,
                               (float*)self_k[l], (float*)self_v[l], D, t, cap);
        PK_LAUNCH_CHECK();
        RC(pk_attn_fwd(s.qkv, self_k[l], self_v[l], s.o, s.lse, nullptr, B, H, 1, t + 1, 64, 3LL * D, 3LL * D, cap * D, D,
                       cap * D, D, D, D, 0, scale, 0.f, 0, 0, nullptr, dt, stream));
        RC(linear(s.o, w.out_w, w.out_b, s.q, D, D, PK_ACT_NONE));
        RC(block_end(s.q, w.ln1_g, w.ln1_b));
        // ---- cross-attention over the cached projections of the encoder output ----
        RC(block_in(w.ln2_g, w.ln2_b, &in));
        RC(linear(in, w.cq_w, w.cq_b, s.q, D, D, PK_ACT_NONE));
        const char* ckv = (const char*)cross_kv[l];
        RC(pk_attn_fwd(s.q, ckv, ckv + (size_t)D * es, s.o, s.lse, enc_mask, B, H, 1, S, 64, D, D, (long long)S * 2 * D,
                       2LL * D, (long long)S * 2 * D, 2LL * D, D, D, 0, scale, 0.f, 0, 0, nullptr, dt, stream));
        RC(linear(s.o, w.cout_w, w.cout_b, s.q, D, D, PK_ACT_NONE));
        RC(block_end(s.q, w.ln2_g, w.ln2_b));
        // ---- feed-forward ----
        RC(block_in(w.ln3_g, w.ln3_b, &in));
        if (moe && moe[l].E > 0) {  // (fc1_* / fc2_* of such a layer are NULL)
            RC(pk_moerows(in, s.q, moe[l].gate_w, moe[l].w1, moe[l].b1, moe[l].w2, moe[l].b2, B, moe[l].E, D, moe[l].F, plan->act, dt,
                           s.moe, s.moe_bytes, stream));
        } else {
            RC(linear(in, w.fc1_w, w.fc1_b, s.ff, F, D, plan->act));
            RC(linear(s.ff, w.fc2_w, w.fc2_b, s.q, D, F, PK_ACT_NONE));
        }
        RC(block_end(s.q, w.ln3_g, w.ln3_b));
        // ---- the layer's adapters (AdapterTransformerDecoderLayer.forward): x <- adapter(x), into the other buffer ----
        for (int i = 0; adapters && i < adapters[l].n; ++i) {
            const PkAdapter& ad = adapters[l].a[i];
            RC(pk_adapter_rows_step(x, xn, ad.ln_g, ad.ln_b, ad.down_w, ad.down_b, ad.up_w, ad.up_b, B, D, ad.p, ad.act, ad.scaling,
                               ad.eps, dt, s.ad, s.ad_bytes, stream));
            std::swap(x, xn);
        }
    }
    if (plan->final_ln_g) {
        RC(pk_residual_ln_fwd(x, nullptr, plan->final_ln_g, plan->final_ln_b, nullptr, xn, s.mean, s.rstd, B, D, plan->eps,
                              0.f, 0, 0, dt, stream));
        std::swap(x, xn);
    }
    // output projection (tied: x E^T, modules.py:935-947)
    RC(pk_gemm(x, plan->out_w, logits, nullptr, nullptr, nullptr, B, plan->vocab, D, D, D, ld_logits, 0, 0, 0, 0, PK_ACT_NONE,
               0, 1.f, dt, 1, nullptr, 0, nullptr, stream));
    return 0;
}

extern "C" int pk_decoder_step_ex(const PkDecoderPlan* plan, const long long* ids, int B, int t, int pos_start,
                                  void* const* self_k, void* const* self_v, long long cap, const void* const* cross_kv,
                                  const unsigned char* enc_mask, int S, void* scratch, size_t scratch_bytes, void* logits,
                                  long long ld_logits, const PkAdapterStack* adapters, void* stream) {
    return pk_decoder_step_moe(plan, ids, B, t, pos_start, self_k, self_v, cap, cross_kv, enc_mask, S, scratch, scratch_bytes,
                               logits, ld_logits, adapters, nullptr, stream);
}

extern "C" int pk_decoder_step(const PkDecoderPlan* plan, const long long* ids, int B, int t, int pos_start,
                               void* const* self_k, void* const* self_v, long long cap, const void* const* cross_kv,
                               const unsigned char* enc_mask, int S, void* scratch, size_t scratch_bytes, void* logits,
                               long long ld_logits, void* stream) {
    return pk_decoder_step_ex(plan, ids, B, t, pos_start, self_k, self_v, cap, cross_kv, enc_mask, S, scratch, scratch_bytes,
                              logits, ld_logits, nullptr, stream);
}

extern "C" int pk_argmax_rows(const void* x, long long rows, long long n, long long ld, long long* out,
                              long long out_stride, int dtype, void* stream) {
    PK_CHECK_ARG(x && out && n > 0 && ld >= n, "pk_argmax_rows: bad arguments");
    if (rows == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == PK_BF16)
        hipLaunchKernelGGL((argmax_rows_kernel<bf16>), dim3((unsigned)rows), dim3(256), 0, st, (const bf16*)x, ld, n, out, out_stride);
    else if (dtype == PK_F16)
        hipLaunchKernelGGL((argmax_rows_kernel<f16>), dim3((unsigned)rows), dim3(256), 0, st, (const f16*)x, ld, n, out, out_stride);
    else if (dtype == PK_F32)
        hipLaunchKernelGGL((argmax_rows_kernel<float>), dim3((unsigned)rows), dim3(256), 0, st, (const float*)x, ld, n, out, out_stride);
    else PK_CHECK_ARG(false, "pk_argmax_rows: dtype %d not supported", dtype);
    PK_LAUNCH_CHECK();
    return 0;
}
