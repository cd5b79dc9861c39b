// Mixture-of-experts feed-forward (pasero/models/mixture_of_experts.py, the `basic` semantics with an fp32 gate) as ROUTED
// computation: every token runs through its two experts only, nothing reads back to the host.
//
//   pk_moe_gate      softmax over E, top-2, normalised weights, load-balancing statistics and the routing tables
//   pk_moe_gate_bwd  d logits from d top_w and the load-balancing term (normalisation, mask, softmax)
//   pk_moe_gather    Xg[slot] = X[token_of[slot]] (* top_w of that pair)          token order -> slot order
//   pk_moe_combine   out[token] = sum_k top_w[k] * Y[slot_of[token][k]]           slot order -> token order, no atomics
//   pk_moe_dot       d top_w[token][k] = <dOut[token], Y[slot_of[token][k]]>
//   pk_moe_gemm      one launch for all experts: expert e owns rows offsets[e] .. offsets[e+1] of the slot-ordered buffers
//   pk_moe_gemm_wgrad  dW_e = dY_e^T X_e, db_e = colsum(dY_e): the contraction length is the expert's row count
//
// Ranking rule (documented difference from torch.topk, which leaves ties open): experts are ranked by their fp32 gate
// VALUE (after the softmax), higher first; among exactly equal fp32 values the LOWER expert index wins.
//
// Routing tables: the (token, k) pairs of the real (non-padding) tokens sorted by expert, then token, then k — a stable
// counting sort over chunks of 256 tokens: per-chunk counts, one scan, per-chunk placement by rank.  Integer arithmetic
// and fixed-order float sums only: two calls give the same bits.
//
// Grouped GEMM: the grid is sized from the capacity 2S and E alone — ceil(2S / 128) + E row tiles cover every distribution
// (sum_e ceil(n_e / 128) <= 2S / 128 + E); a workgroup walks `offsets` (device memory) to find its expert and row tile,
// surplus workgroups exit.  16-bit types: 128 x 128 tile, 4 waves of 64 x 64 (2 x 2 v_mfma_f32_32x32x16), BK = 32, both
// operands staged k-contiguous in LDS (col-form operands are transposed on the way in), the next K-tile's global loads
// in flight under the MFMAs.  fp32: one thread per output element (exists for the parity tests).  Rows at and beyond
// offsets[E] are neither read nor written.
#include <cstdlib>
#include "common.h"
#include "moe_gate.h"

namespace {

constexpr int GATE_CHUNK = 256;  // tokens per counting-sort chunk
// one wave per token (the softmax and the top-2 choice: moe_gate.h, shared with the few-rows route kernel of moe_rows.hip)
__global__ __launch_bounds__(256) void gate_rows_kernel(const float* __restrict__ logits, const unsigned char* __restrict__ pad,
                                                        long long S, int E, float* __restrict__ gv, int* __restrict__ top_idx,
                                                        float* __restrict__ top_w) {
    const long long s = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (s >= S) return;
    const bool is_pad = pad != nullptr && pad[s] != 0;
    float* g_row = gv + s * E;
    if (is_pad) {
        for (int e = lane; e < E; e += 64) g_row[e] = 0.f;
        if (lane < 2) {
            top_idx[2 * s + lane] = -1;
            top_w[2 * s + lane] = 0.f;
        }
        return;
    }
    int bi[2];
    float bw[2];
    const float* row = logits + s * E;
    moe_gate_token([row](int e) { return row[e]; }, lane, E, g_row, bi, bw);
    if (lane == 0) {
        top_idx[2 * s] = bi[0];
        top_idx[2 * s + 1] = bi[1];
        top_w[2 * s] = bw[0];
        top_w[2 * s + 1] = bw[1];
    }
}

// per chunk: pair counts, top-1 counts and gate-value sums per expert
__global__ __launch_bounds__(GATE_CHUNK) void gate_count_kernel(const float* __restrict__ gv, const int* __restrict__ top_idx,
                                                                long long S, int E, int* __restrict__ cnt,
                                                                int* __restrict__ cnt1, float* __restrict__ psum) {
    __shared__ int c[MOE_E_MAX], c1[MOE_E_MAX];
    const int tid = threadIdx.x;
    const long long t0 = (long long)blockIdx.x * GATE_CHUNK;
    c[tid] = 0;
    c1[tid] = 0;
    __syncthreads();
    const long long s = t0 + tid;
    if (s < S) {
        const int i1 = top_idx[2 * s], i2 = top_idx[2 * s + 1];
        if (i1 >= 0) {
            atomicAdd(&c[i1], 1);
            atomicAdd(&c1[i1], 1);
            atomicAdd(&c[i2], 1);
        }
    }
    __syncthreads();
    if (tid < E) {
        const long long o = (long long)blockIdx.x * E + tid;
        cnt[o] = c[tid];
        cnt1[o] = c1[tid];
        float p = 0.f;
        const long long t1 = t0 + GATE_CHUNK < S ? t0 + GATE_CHUNK : S;
        for (long long t = t0; t < t1; ++t) p += gv[t * E + tid];
        psum[o] = p;
    }
}

// one workgroup: chunk bases (exclusive scan over the chunks, in place), expert offsets, statistics, load-balancing term
__global__ __launch_bounds__(MOE_E_MAX) void gate_scan_kernel(int nchunk, int E, int* __restrict__ cnt, const int* __restrict__ cnt1,
                                                              const float* __restrict__ psum, int* __restrict__ offsets,
                                                              int* __restrict__ top1_count, float* __restrict__ prob_sum,
                                                              float* __restrict__ lb_coef, float* __restrict__ lb_loss) {
    __shared__ int tot[MOE_E_MAX];
    __shared__ float term[MOE_E_MAX];
    __shared__ int total;
    const int e = threadIdx.x;
    int n1 = 0;
    float p = 0.f;
    if (e < E) {
        int run = 0;
        for (int ch = 0; ch < nchunk; ++ch) {
            const long long o = (long long)ch * E + e;
            const int t = cnt[o];
            cnt[o] = run;
            run += t;
            n1 += cnt1[o];
            p += psum[o];
        }
        tot[e] = run;
        top1_count[e] = n1;
        prob_sum[e] = p;
    }
    __syncthreads();
    if (e == 0) {
        int off = 0;
        for (int i = 0; i < E; ++i) {
            offsets[i] = off;
            off += tot[i];
        }
        offsets[E] = off;
        total = off;
    }
    __syncthreads();
    const float nt = (float)(total / 2);  // real tokens
    if (e < E) {
        // lb_loss = E * sum_e (top1_e / nt) * (prob_sum_e / nt); its derivative w.r.t. a real token's gate value of expert e
        const float frac = nt > 0.f ? (float)n1 / nt : 0.f;
        lb_coef[e] = nt > 0.f ? (float)E * frac / nt : 0.f;
        term[e] = nt > 0.f ? frac * (p / nt) : 0.f;
    }
    __syncthreads();
    if (e == 0) {
        float l = 0.f;
        for (int i = 0; i < E; ++i) l += term[i];
        lb_loss[0] = (float)E * l;
    }
}

// per chunk: the slot of every pair = offsets[expert] + chunk base + rank among the chunk's earlier pairs of that expert
__global__ __launch_bounds__(GATE_CHUNK) void gate_place_kernel(const int* __restrict__ top_idx, long long S, int E,
                                                                const int* __restrict__ base, const int* __restrict__ offsets,
                                                                int* __restrict__ slot_of, int* __restrict__ token_of) {
    __shared__ int idx[2 * GATE_CHUNK];
    const int tid = threadIdx.x;
    const long long s = (long long)blockIdx.x * GATE_CHUNK + tid;
    int i1 = -1, i2 = -1;
    if (s < S) {
        i1 = top_idx[2 * s];
        i2 = top_idx[2 * s + 1];
    }
    idx[2 * tid] = i1;
    idx[2 * tid + 1] = i2;
    __syncthreads();
    if (s >= S) return;
    if (i1 < 0) {
        slot_of[2 * s] = -1;
        slot_of[2 * s + 1] = -1;
        return;
    }
    int r1 = 0, r2 = 0;
    for (int p = 0; p < 2 * tid; ++p) {
        const int v = idx[p];
        r1 += v == i1;
        r2 += v == i2;
    }
    const int* b = base + (long long)blockIdx.x * E;
    const int s1 = offsets[i1] + b[i1] + r1, s2 = offsets[i2] + b[i2] + r2;
    slot_of[2 * s] = s1;
    slot_of[2 * s + 1] = s2;
    token_of[s1] = (int)s;
    token_of[s2] = (int)s;
}

// one wave per token
__global__ __launch_bounds__(256) void gate_bwd_kernel(const float* __restrict__ d_top_w, const float* __restrict__ lb_coef,
                                                       const float* __restrict__ scale_dev, float scale_host,
                                                       const float* __restrict__ gv, const int* __restrict__ top_idx,
                                                       float* __restrict__ d_logits, long long S, int E) {
    const long long s = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (s >= S) return;
    const int i1 = top_idx[2 * s], i2 = top_idx[2 * s + 1];
    float* out = d_logits + s * E;
    if (i1 < 0) {
        for (int e = lane; e < E; e += 64) out[e] = 0.f;
        return;
    }
    const float scale = lb_coef != nullptr ? scale_host * (scale_dev != nullptr ? scale_dev[0] : 1.f) : 0.f;
    const float* g = gv + s * E;
    const float g1 = g[i1], g2 = g[i2], den = g1 + g2;
    float dg1 = 0.f, dg2 = 0.f;
    if (d_top_w != nullptr) {
        // w_k = g_k / (g_1 + g_2):  d g_k = (d w_k - (d w_1 w_1 + d w_2 w_2)) / (g_1 + g_2)
        const float dw1 = d_top_w[2 * s], dw2 = d_top_w[2 * s + 1];
        const float dot = (dw1 * g1 + dw2 * g2) / den;
        dg1 = (dw1 - dot) / den;
        dg2 = (dw2 - dot) / den;
    }
    float dg[4], gg[4];
    float inner = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int e = lane + 64 * j;
        gg[j] = 0.f;
        dg[j] = 0.f;
        if (e < E) {
            gg[j] = g[e];
            dg[j] = (lb_coef != nullptr ? scale * lb_coef[e] : 0.f) + (e == i1 ? dg1 : 0.f) + (e == i2 ? dg2 : 0.f);
            inner += gg[j] * dg[j];
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) inner += __shfl_xor(inner, o, 64);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int e = lane + 64 * j;
        if (e < E) out[e] = gg[j] * (dg[j] - inner);
    }
}

// ---- token order <-> slot order ----
template <typename T>
__global__ __launch_bounds__(256) void gather_kernel(const T* __restrict__ X, T* __restrict__ Xg, const int* __restrict__ token_of,
                                                     const int* __restrict__ offsets, const int* __restrict__ slot_of,
                                                     const float* __restrict__ top_w, int E, int D) {
    constexpr int EPV = 16 / sizeof(T);
    const int slot = blockIdx.x;
    if (slot >= offsets[E]) return;
    const int token = token_of[slot];
    float w = 1.f;
    if (top_w != nullptr) w = top_w[2 * (long long)token + (slot_of[2 * (long long)token] == slot ? 0 : 1)];
    const T* src = X + (long long)token * D;
    T* dst = Xg + (long long)slot * D;
    for (int c = threadIdx.x * EPV; c < D; c += blockDim.x * EPV) {
        Vec16<T> v = load16<T>(src + c);
        if (top_w != nullptr) {
            float f[EPV];
#pragma unroll
            for (int i = 0; i < EPV; ++i) f[i] = v.get(i) * w;
            v = vec16_pack<T>(f);
        }
        store16<T>(dst + c, v);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void combine_kernel(const T* __restrict__ Y, T* __restrict__ out, const int* __restrict__ slot_of,
                                                      const float* __restrict__ top_w, int D) {
    constexpr int EPV = 16 / sizeof(T);
    const long long token = blockIdx.x;
    const int s0 = slot_of[2 * token], s1 = slot_of[2 * token + 1];
    const float w0 = top_w != nullptr ? top_w[2 * token] : 1.f, w1 = top_w != nullptr ? top_w[2 * token + 1] : 1.f;
    T* dst = out + token * D;
    for (int c = threadIdx.x * EPV; c < D; c += blockDim.x * EPV) {
        float f[EPV];
#pragma unroll
        for (int i = 0; i < EPV; ++i) f[i] = 0.f;
        if (s0 >= 0) {  // (padding tokens: exactly 0)
            const Vec16<T> a = load16<T>(Y + (long long)s0 * D + c), b = load16<T>(Y + (long long)s1 * D + c);
#pragma unroll
            for (int i = 0; i < EPV; ++i) f[i] = w0 * a.get(i) + w1 * b.get(i);
        }
        store16<T>(dst + c, vec16_pack<T>(f));
    }
}

template <typename T>
__global__ __launch_bounds__(256) void dot_kernel(const T* __restrict__ dOut, const T* __restrict__ Y, const int* __restrict__ slot_of,
                                                  float* __restrict__ d_top_w, int D) {
    constexpr int EPV = 16 / sizeof(T);
    __shared__ float red[2][4];
    const long long token = blockIdx.x;
    const int s0 = slot_of[2 * token], s1 = slot_of[2 * token + 1];
    if (s0 < 0) {
        if (threadIdx.x < 2) d_top_w[2 * token + threadIdx.x] = 0.f;
        return;
    }
    float a0 = 0.f, a1 = 0.f;
    for (int c = threadIdx.x * EPV; c < D; c += blockDim.x * EPV) {
        const Vec16<T> g = load16<T>(dOut + token * D + c);
        const Vec16<T> y0 = load16<T>(Y + (long long)s0 * D + c), y1 = load16<T>(Y + (long long)s1 * D + c);
#pragma unroll
        for (int i = 0; i < EPV; ++i) {
            a0 += g.get(i) * y0.get(i);
            a1 += g.get(i) * y1.get(i);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a0 += __shfl_xor(a0, o, 64);
        a1 += __shfl_xor(a1, o, 64);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red[0][wave] = a0;
        red[1][wave] = a1;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const float* r = red[threadIdx.x];
        d_top_w[2 * token + threadIdx.x] = (r[0] + r[1]) + (r[2] + r[3]);
    }
}

// ---- grouped GEMM ----
struct MoeGemmArgs {
    const void* A;            // slot-ordered [rows][lda]
    const void* X;            // weight gradient: the second slot-ordered operand [rows][ldb]
    const void* const* W;     // forward / dX: E weight pointers
    const void* const* bias;  // forward: E bias pointers, or NULL
    void* C;                  // forward / dX: slot-ordered output [rows][N]
    void* const* dW;          // weight gradient: E output pointers [M][N]
    const void* aux;          // mode 2: [rows][N]
    void* preact;             // mode 0, optional: [rows][N]
    const int* offsets;
    int E, act, mode;
    long long M, N, K;        // forward / dX: N output columns, K contraction; weight gradient: M x N outputs
};

constexpr int GB = 128, GK = 32, GP = GK + 8;  // tile, K-step, LDS row pitch (16-bit elements; 80 B keeps 16-B alignment)

// which (expert, row tile) workgroup `t` of a forward / dX launch works on; false: a surplus workgroup
template <int TILE>
__device__ __forceinline__ bool find_tile(const int* __restrict__ offsets, int E, int t, int& e_out, int& r0, int& r1) {
    for (int e = 0; e < E; ++e) {
        const int b = offsets[e], n = offsets[e + 1] - b;
        const int tiles = (n + TILE - 1) / TILE;
        if (t < tiles) {
            e_out = e;
            r0 = b + t * TILE;
            r1 = b + n;
            return true;
        }
        t -= tiles;
    }
    return false;
}

// stage one 128 x 32 operand tile into registers.  Row form: memory [row][ld], k contiguous.  Col form: memory [k][ld], the
// tile's row index contiguous.  Out-of-range chunks read as zero (every extent is a multiple of 8 except the slot rows).
template <typename T, bool COL>
__device__ __forceinline__ void stage_load(uint4 (&v)[2], const T* __restrict__ base, long long ld, long long row0, long long row_lim,
                                           long long k0, long long k_lim, int tid) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int c = tid + i * 256;
        v[i] = uint4{0, 0, 0, 0};
        if constexpr (!COL) {
            const long long r = row0 + (c >> 2), k = k0 + (c & 3) * 8;
            if (r < row_lim && k < k_lim) v[i] = *reinterpret_cast<const uint4*>(base + r * ld + k);
        } else {
            const long long k = k0 + (c >> 4), r = row0 + (c & 15) * 8;
            if (k < k_lim && r < row_lim) v[i] = *reinterpret_cast<const uint4*>(base + k * ld + r);
        }
    }
}
template <bool COL>
__device__ __forceinline__ void stage_store(const uint4 (&v)[2], unsigned short* lds, int tid) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int c = tid + i * 256;
        if constexpr (!COL) {
            *reinterpret_cast<uint4*>(lds + (c >> 2) * GP + (c & 3) * 8) = v[i];
        } else {
            const int k = c >> 4, r = (c & 15) * 8;
            const unsigned w[4] = {v[i].x, v[i].y, v[i].z, v[i].w};
#pragma unroll
            for (int j = 0; j < 8; ++j) lds[(r + j) * GP + k] = (unsigned short)(w[j >> 1] >> ((j & 1) * 16));
        }
    }
}

// FORM 0: C_e = epi(A_e W_e^T)   (W_e [N][K])     FORM 1: C_e = epi(A_e W_e)   (W_e [K][N])
// FORM 2: dW_e [M][N] = A_e^T X_e   (A = dY [rows][M], X [rows][N]; contraction over the expert's rows)
template <typename T, int FORM>
__global__ __launch_bounds__(256) void moe_gemm16_kernel(MoeGemmArgs p) {
    __shared__ __attribute__((aligned(16))) unsigned short sa[GB * GP];
    __shared__ __attribute__((aligned(16))) unsigned short sb[GB * GP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    int e, r0 = 0, r1 = 0;
    // forward / dX: the row tiles, whose number grows with the batch, are grid.x (2^31 - 1 workgroups), the column tiles grid.y
    long long m0, n0 = (long long)(FORM == 2 ? blockIdx.x : blockIdx.y) * GB;
    if constexpr (FORM == 2) {
        e = blockIdx.z;
        m0 = (long long)blockIdx.y * GB;
        r0 = p.offsets[e];
        r1 = p.offsets[e + 1];
    } else {
        if (!find_tile<GB>(p.offsets, p.E, blockIdx.x, e, r0, r1)) return;
        m0 = r0;
    }
    const T* A = reinterpret_cast<const T*>(p.A);
    const T* B = FORM == 2 ? reinterpret_cast<const T*>(p.X) : reinterpret_cast<const T*>(p.W[e]);
    // contraction range, leading dimensions and row limits of the two operands
    const long long kb = FORM == 2 ? r0 : 0, ke = FORM == 2 ? r1 : p.K;
    const long long lda = FORM == 2 ? p.M : p.K;
    const long long ldb = FORM == 0 ? p.K : p.N;
    const long long a_lim = FORM == 2 ? p.M : r1, b_lim = p.N;
    constexpr bool A_COL = FORM == 2, B_COL = FORM != 0;

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[i][j][v] = 0.f;

    uint4 ra[2], rb[2];
    if (kb < ke) {
        stage_load<T, A_COL>(ra, A, lda, m0, a_lim, kb, ke, tid);
        stage_load<T, B_COL>(rb, B, ldb, n0, b_lim, kb, ke, tid);
    }
    for (long long k0 = kb; k0 < ke; k0 += GK) {
        __syncthreads();
        stage_store<A_COL>(ra, sa, tid);
        stage_store<B_COL>(rb, sb, tid);
        __syncthreads();
        if (k0 + GK < ke) {
            stage_load<T, A_COL>(ra, A, lda, m0, a_lim, k0 + GK, ke, tid);
            stage_load<T, B_COL>(rb, B, ldb, n0, b_lim, k0 + GK, ke, tid);
        }
#pragma unroll
        for (int kk = 0; kk < GK / 16; ++kk) {
            typename H16<T>::vec fa[2], fb[2];
            const int ko = kk * 16 + (lane >> 5) * 8;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                fa[i] = *reinterpret_cast<const typename H16<T>::vec*>(sa + (wm * 64 + i * 32 + (lane & 31)) * GP + ko);
                fb[i] = *reinterpret_cast<const typename H16<T>::vec*>(sb + (wn * 64 + i * 32 + (lane & 31)) * GP + ko);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = H16<T>::mfma(fa[i], fb[j], acc[i][j]);
        }
    }

    // epilogue from the accumulators: lane l holds column l & 31 of rows 8 * (v / 4) + 4 * (l >> 5) + v % 4
    const long long m_lim = FORM == 2 ? p.M : r1;
    T* C = FORM == 2 ? reinterpret_cast<T*>(p.dW[e]) : reinterpret_cast<T*>(p.C);
    const T* bias = (FORM == 0 && p.bias != nullptr) ? reinterpret_cast<const T*>(p.bias[e]) : nullptr;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const long long n = n0 + wn * 64 + j * 32 + (lane & 31);
        if (n >= p.N) continue;
        const float bn = bias != nullptr ? to_f32<T>(bias[n]) : 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const long long m = m0 + wm * 64 + i * 32 + 8 * (v >> 2) + 4 * (lane >> 5) + (v & 3);
                if (m >= m_lim) continue;
                const long long o = m * p.N + n;
                float x = acc[i][j][v];
                if (FORM != 2) {
                    if (p.mode == 2) {
                        x *= act_bwd_t<T>(p.act, to_f32<T>(reinterpret_cast<const T*>(p.aux)[o]));
                    } else {
                        x += bn;
                        if (p.preact != nullptr) reinterpret_cast<T*>(p.preact)[o] = from_f32<T>(x);
                        x = act_fwd_t<T>(p.act, x);
                    }
                }
                C[o] = from_f32<T>(x);
            }
        }
    }
}

// fp32 (and the reference form of the above): one thread per output element, 16 x 16 outputs per workgroup
template <typename T, int FORM>
__global__ __launch_bounds__(256) void moe_gemm_plain_kernel(MoeGemmArgs p) {
    int e, r0 = 0, r1 = 0;
    long long m;
    const long long n = (long long)(FORM == 2 ? blockIdx.x : blockIdx.y) * 16 + threadIdx.x;
    if constexpr (FORM == 2) {
        e = blockIdx.z;
        m = (long long)blockIdx.y * 16 + threadIdx.y;
        r0 = p.offsets[e];
        r1 = p.offsets[e + 1];
        if (m >= p.M || n >= p.N) return;
    } else {
        if (!find_tile<16>(p.offsets, p.E, blockIdx.x, e, r0, r1)) return;
        m = r0 + threadIdx.y;
        if (m >= r1 || n >= p.N) return;
    }
    const T* A = reinterpret_cast<const T*>(p.A);
    float acc = 0.f;
    if constexpr (FORM == 0) {
        const T* a = A + m * p.K;
        const T* w = reinterpret_cast<const T*>(p.W[e]) + n * p.K;
        for (long long k = 0; k < p.K; ++k) acc = fmaf(to_f32<T>(a[k]), to_f32<T>(w[k]), acc);
    } else if constexpr (FORM == 1) {
        const T* a = A + m * p.K;
        const T* w = reinterpret_cast<const T*>(p.W[e]) + n;
        for (long long k = 0; k < p.K; ++k) acc = fmaf(to_f32<T>(a[k]), to_f32<T>(w[k * p.N]), acc);
    } else {
        const T* x = reinterpret_cast<const T*>(p.X);
        for (long long r = r0; r < r1; ++r) acc = fmaf(to_f32<T>(A[r * p.M + m]), to_f32<T>(x[r * p.N + n]), acc);
    }
    const long long o = m * p.N + n;
    if constexpr (FORM == 2) {
        reinterpret_cast<T*>(p.dW[e])[o] = from_f32<T>(acc);
    } else {
        float x = acc;
        if (p.mode == 2) {
            x *= act_bwd_t<T>(p.act, to_f32<T>(reinterpret_cast<const T*>(p.aux)[o]));
        } else {
            if (p.bias != nullptr) x += to_f32<T>(reinterpret_cast<const T*>(p.bias[e])[n]);
            if (p.preact != nullptr) reinterpret_cast<T*>(p.preact)[o] = from_f32<T>(x);
            x = act_fwd_t<T>(p.act, x);
        }
        reinterpret_cast<T*>(p.C)[o] = from_f32<T>(x);
    }
}

// db_e[m] = sum over the expert's rows of dY[r][m], in row order (fixed order: deterministic)
template <typename T>
__global__ __launch_bounds__(256) void moe_colsum_kernel(const T* __restrict__ dY, void* const* __restrict__ db,
                                                         const int* __restrict__ offsets, long long M) {
    const int e = blockIdx.y;
    const long long m = (long long)blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    float s = 0.f, comp = 0.f;  // compensated (Kahan): a long column of one expert sums to within an ulp or two of fp32
    for (int r = offsets[e]; r < offsets[e + 1]; ++r) {
        const float y = to_f32<T>(dY[(long long)r * M + m]) - comp;
        const float t = s + y;
        comp = (t - s) - y;
        s = t;
    }
    reinterpret_cast<T*>(db[e])[m] = from_f32<T>(s);
}

int g_use_grouped = -1;

}  // namespace

extern "C" {

size_t pk_moe_gate_scratch(long long S, int E) {
    if (S < 1 || E < 2 || E > MOE_E_MAX) return 0;
    const long long nchunk = (S + GATE_CHUNK - 1) / GATE_CHUNK;
    return (size_t)nchunk * E * 3 * 4;
}

int pk_moe_gate(const float* logits, const unsigned char* pad, long long S, int E, float* gate_value, int* top_idx,
                float* top_w, int* top1_count, float* prob_sum, float* lb_coef, float* lb_loss, int* offsets, int* slot_of,
                int* token_of, void* scratch, size_t scratch_bytes, void* stream) {
    PK_CHECK_ARG(E >= 2 && E <= MOE_E_MAX, "pk_moe_gate: expert count %d outside [2, %d]", E, MOE_E_MAX);
    PK_CHECK_ARG(S >= 1 && S < (1LL << 29), "pk_moe_gate: token count %lld outside [1, 2^29)", S);
    PK_CHECK_ARG(logits && gate_value && top_idx && top_w, "pk_moe_gate: null logits / gate_value / top_idx / top_w");
    PK_CHECK_ARG(top1_count && prob_sum && lb_coef && lb_loss, "pk_moe_gate: null statistics output");
    PK_CHECK_ARG(offsets && slot_of && token_of, "pk_moe_gate: null routing table");
    const size_t need = pk_moe_gate_scratch(S, E);
    PK_CHECK_ARG(scratch && scratch_bytes >= need, "pk_moe_gate: scratch of %zu bytes, %zu needed", scratch ? scratch_bytes : 0, need);
    hipStream_t st = (hipStream_t)stream;
    const int nchunk = (int)((S + GATE_CHUNK - 1) / GATE_CHUNK);
    int* cnt = (int*)scratch;
    int* cnt1 = cnt + (size_t)nchunk * E;
    float* psum = (float*)(cnt1 + (size_t)nchunk * E);
    gate_rows_kernel<<<dim3((unsigned)((S + 3) / 4)), 256, 0, st>>>(logits, pad, S, E, gate_value, top_idx, top_w);
    PK_LAUNCH_CHECK();
    gate_count_kernel<<<nchunk, GATE_CHUNK, 0, st>>>(gate_value, top_idx, S, E, cnt, cnt1, psum);
    PK_LAUNCH_CHECK();
    gate_scan_kernel<<<1, MOE_E_MAX, 0, st>>>(nchunk, E, cnt, cnt1, psum, offsets, top1_count, prob_sum, lb_coef, lb_loss);
    PK_LAUNCH_CHECK();
    gate_place_kernel<<<nchunk, GATE_CHUNK, 0, st>>>(top_idx, S, E, cnt, offsets, slot_of, token_of);
    PK_LAUNCH_CHECK();
    return 0;
}

int pk_moe_gate_bwd(const float* d_top_w, const float* lb_coef, const float* lb_scale_dev, float lb_scale,
                    const float* gate_value, const int* top_idx, float* d_logits, long long S, int E, void* stream) {
    PK_CHECK_ARG(E >= 2 && E <= MOE_E_MAX, "pk_moe_gate_bwd: expert count %d outside [2, %d]", E, MOE_E_MAX);
    PK_CHECK_ARG(S >= 1 && S < (1LL << 29), "pk_moe_gate_bwd: token count %lld outside [1, 2^29)", S);
    PK_CHECK_ARG(gate_value && top_idx && d_logits, "pk_moe_gate_bwd: null gate_value / top_idx / d_logits");
    gate_bwd_kernel<<<dim3((unsigned)((S + 3) / 4)), 256, 0, (hipStream_t)stream>>>(d_top_w, lb_coef, lb_scale_dev, lb_scale,
                                                                                   gate_value, top_idx, d_logits, S, E);
    PK_LAUNCH_CHECK();
    return 0;
}

#define PK_MOE_ROW_CHECKS(who, S, E, D)                                                                  \
    PK_CHECK_ARG(E >= 2 && E <= MOE_E_MAX, who ": expert count %d outside [2, %d]", E, MOE_E_MAX);       \
    PK_CHECK_ARG(S >= 1 && S < (1LL << 29), who ": token count %lld outside [1, 2^29)", (long long)(S)); \
    PK_CHECK_ARG(D >= 8 && D % 8 == 0, who ": row width %d is not a positive multiple of 8", D)

int pk_moe_gather(const void* X, void* Xg, const int* token_of, const int* offsets, const int* slot_of, const float* top_w,
                  long long S, int E, int D, int dtype, void* stream) {
    PK_MOE_ROW_CHECKS("pk_moe_gather", S, E, D);
    PK_CHECK_ARG(X && Xg && token_of && offsets, "pk_moe_gather: null buffer or routing table");
    PK_CHECK_ARG(top_w == nullptr || slot_of != nullptr, "pk_moe_gather: a per-slot scale needs slot_of");
    PK_DTYPE_SWITCH(dtype, "pk_moe_gather", {
        gather_kernel<T><<<dim3((unsigned)(2 * S)), 256, 0, (hipStream_t)stream>>>((const T*)X, (T*)Xg, token_of, offsets, slot_of,
                                                                                  top_w, E, D);
    })
    PK_LAUNCH_CHECK();
    return 0;
}

int pk_moe_combine(const void* Y, void* out, const int* slot_of, const float* top_w, long long S, int D, int dtype,
                   void* stream) {
    PK_MOE_ROW_CHECKS("pk_moe_combine", S, 2, D);
    PK_CHECK_ARG(Y && out && slot_of, "pk_moe_combine: null buffer or routing table");
    PK_DTYPE_SWITCH(dtype, "pk_moe_combine", {
        combine_kernel<T><<<dim3((unsigned)S), 256, 0, (hipStream_t)stream>>>((const T*)Y, (T*)out, slot_of, top_w, D);
    })
    PK_LAUNCH_CHECK();
    return 0;
}

int pk_moe_dot(const void* dOut, const void* Y, const int* slot_of, float* d_top_w, long long S, int D, int dtype,
               void* stream) {
    PK_MOE_ROW_CHECKS("pk_moe_dot", S, 2, D);
    PK_CHECK_ARG(dOut && Y && slot_of && d_top_w, "pk_moe_dot: null buffer or routing table");
    PK_DTYPE_SWITCH(dtype, "pk_moe_dot", {
        dot_kernel<T><<<dim3((unsigned)S), 256, 0, (hipStream_t)stream>>>((const T*)dOut, (const T*)Y, slot_of, d_top_w, D);
    })
    PK_LAUNCH_CHECK();
    return 0;
}

int pk_moe_gemm(const void* A, const void* const* W, const void* const* bias, void* C, const void* aux, void* preact,
                const int* offsets, long long rows, int E, long long N, long long K, int b_col, int act, int mode, int dtype,
                void* stream) {
    PK_CHECK_ARG(E >= 2 && E <= MOE_E_MAX, "pk_moe_gemm: expert count %d outside [2, %d]", E, MOE_E_MAX);
    PK_CHECK_ARG(rows >= 1 && rows < (1LL << 30), "pk_moe_gemm: %lld slot rows outside [1, 2^30)", rows);
    PK_CHECK_ARG(N >= 8 && K >= 8 && N % 8 == 0 && K % 8 == 0, "pk_moe_gemm: N = %lld, K = %lld: D and F must be multiples of 8", N, K);
    PK_CHECK_ARG(N <= (1 << 19) && K <= (1 << 19), "pk_moe_gemm: N = %lld, K = %lld beyond 2^19 columns", N, K);
    PK_CHECK_ARG(A && W && C && offsets, "pk_moe_gemm: null operand, pointer table or offsets");
    PK_CHECK_ARG(mode == 0 || mode == 2, "pk_moe_gemm: epilogue mode %d (0 or 2)", mode);
    PK_CHECK_ARG(mode != 2 || (aux != nullptr && bias == nullptr && preact == nullptr), "pk_moe_gemm: mode 2 takes aux and neither bias nor preact");
    PK_CHECK_ARG(act >= PK_ACT_NONE && act <= PK_ACT_SILU, "pk_moe_gemm: activation %d", act);
    MoeGemmArgs p{};
    p.A = A; p.W = W; p.bias = bias; p.C = C; p.aux = aux; p.preact = preact; p.offsets = offsets;
    p.E = E; p.act = act; p.mode = mode; p.N = N; p.K = K;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == PK_F32) {
        dim3 grid((unsigned)((rows + 15) / 16 + E), (unsigned)((N + 15) / 16));
        if (b_col) moe_gemm_plain_kernel<float, 1><<<grid, dim3(16, 16), 0, st>>>(p);
        else moe_gemm_plain_kernel<float, 0><<<grid, dim3(16, 16), 0, st>>>(p);
    } else if (dtype == PK_BF16 || dtype == PK_F16) {
        dim3 grid((unsigned)((rows + GB - 1) / GB + E), (unsigned)((N + GB - 1) / GB));
        if (dtype == PK_BF16) {
            if (b_col) moe_gemm16_kernel<bf16, 1><<<grid, 256, 0, st>>>(p);
            else moe_gemm16_kernel<bf16, 0><<<grid, 256, 0, st>>>(p);
        } else {
            if (b_col) moe_gemm16_kernel<f16, 1><<<grid, 256, 0, st>>>(p);
            else moe_gemm16_kernel<f16, 0><<<grid, 256, 0, st>>>(p);
        }
    } else {
        PK_CHECK_ARG(false, "pk_moe_gemm: dtype %d not supported", dtype);
    }
    PK_LAUNCH_CHECK();
    return 0;
}

int pk_moe_gemm_wgrad(const void* dY, const void* X, void* const* dW, void* const* db, const int* offsets, long long rows,
                      int E, long long M, long long N, int dtype, void* stream) {
    PK_CHECK_ARG(E >= 2 && E <= MOE_E_MAX, "pk_moe_gemm_wgrad: expert count %d outside [2, %d]", E, MOE_E_MAX);
    PK_CHECK_ARG(rows >= 1 && rows < (1LL << 30), "pk_moe_gemm_wgrad: %lld slot rows outside [1, 2^30)", rows);
    PK_CHECK_ARG(M >= 8 && N >= 8 && M % 8 == 0 && N % 8 == 0, "pk_moe_gemm_wgrad: M = %lld, N = %lld: D and F must be multiples of 8", M, N);
    PK_CHECK_ARG(M <= (1 << 19) && N <= (1 << 19), "pk_moe_gemm_wgrad: M = %lld, N = %lld beyond 2^19 columns", M, N);
    PK_CHECK_ARG(dY && offsets && (dW == nullptr || X != nullptr) && (dW || db), "pk_moe_gemm_wgrad: null operand, pointer table or offsets");
    MoeGemmArgs p{};
    p.A = dY; p.X = X; p.dW = dW; p.offsets = offsets; p.E = E; p.M = M; p.N = N;
    hipStream_t st = (hipStream_t)stream;
    PK_CHECK_ARG(dtype == PK_F32 || dtype == PK_BF16 || dtype == PK_F16, "pk_moe_gemm_wgrad: dtype %d not supported", dtype);
    if (dW != nullptr) {
        if (dtype == PK_F32) {
            moe_gemm_plain_kernel<float, 2><<<dim3((unsigned)((N + 15) / 16), (unsigned)((M + 15) / 16), E), dim3(16, 16), 0, st>>>(p);
        } else {
            dim3 grid((unsigned)((N + GB - 1) / GB), (unsigned)((M + GB - 1) / GB), E);
            if (dtype == PK_BF16) moe_gemm16_kernel<bf16, 2><<<grid, 256, 0, st>>>(p);
            else moe_gemm16_kernel<f16, 2><<<grid, 256, 0, st>>>(p);
        }
        PK_LAUNCH_CHECK();
    }
    if (db != nullptr) {
        dim3 grid((unsigned)((M + 255) / 256), E);
        PK_DTYPE_SWITCH(dtype, "pk_moe_gemm_wgrad", { moe_colsum_kernel<T><<<grid, 256, 0, st>>>((const T*)dY, db, offsets, M); })
        PK_LAUNCH_CHECK();
    }
    return 0;
}

int pk_moe_use_grouped(int on) {
    if (g_use_grouped < 0) {
        const char* s = getenv("PK_MOE_GROUPED");
        g_use_grouped = (s != nullptr && s[0] == '0') ? 0 : 1;
    }
    const int prev = g_use_grouped;
    if (on >= 0) g_use_grouped = on ? 1 : 0;
    return prev;
}

}  // extern "C"
