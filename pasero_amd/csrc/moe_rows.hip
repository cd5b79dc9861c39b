// The mixture-of-experts feed-forward for the FEW rows of a decoding step (one new token per sentence and beam): the
// inference form of MixtureOfExperts.forward — no padding mask, no load-balancing outputs — in one C call, pk_moerows.
//
// At decoding sizes an expert owns 0-4 rows and the block is pure weight streaming, so the shape is gemm_skinny.hip's, not
// the 128-row tiles of moe.hip:
//   moe_route_rows_kernel   ONE workgroup: logits in the model's dtype -> fp32 softmax, top-2 (moe_gate.h: the code
//                           gate_rows_kernel runs), normalised weights, and the routing tables by a stable counting sort in
//                           LDS.  Bit for bit what pk_moe_gate writes for logits.float() without a padding mask.
//   moe_rows_gemm_kernel    C[slot] = act(A[row(slot)] W_e^T + b_e), grid (column tiles, E): a workgroup of an expert without
//                           slots exits at once; otherwise it walks the expert's slots in chunks of 16 (two chunks per pass
//                           over K) on v_mfma_f32_16x16x32, fragments straight from global memory in MFMA layout (16 bytes
//                           per lane, k contiguous), the k-steps dealt round-robin to the four waves, whose fp32 partials
//                           meet in LDS in a fixed order; bias and activation in fp32, 16-byte stores.  GATHER: the A rows
//                           are addressed through token_of (fc1: no gather launch); otherwise by slot (fc2).
// The weighted combine stays pk_moe_combine.  fp32, many rows and other sizes run the kernels of moe.hip inside the same
// call (the grouped route), bitwise what the module computes.
#include <cstdlib>
#include "common.h"
#include "moe_gate.h"

namespace {

constexpr int ROUTE_THREADS = 1024;

// ---- route: one workgroup of 16 waves, a wave per token at a time ----
template <typename T>
__global__ __launch_bounds__(ROUTE_THREADS) void moe_route_rows_kernel(const T* __restrict__ logits, int rows, int E,
                                                                       int* __restrict__ top_idx, float* __restrict__ top_w,
                                                                       int* __restrict__ offsets, int* __restrict__ slot_of,
                                                                       int* __restrict__ token_of) {
    __shared__ int idx[2 * PK_MOE_ROWS_MAX];  // the expert of pair p = 2 * token + k
    __shared__ int cnt[MOE_E_MAX];
    __shared__ int off[MOE_E_MAX + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int s = wave; s < rows; s += ROUTE_THREADS / 64) {
        const T* row = logits + (long long)s * E;
        int bi[2];
        float bw[2];
        moe_gate_token([row](int e) { return to_f32<T>(row[e]); }, lane, E, nullptr, bi, bw);
        if (lane == 0) {
            idx[2 * s] = bi[0];
            idx[2 * s + 1] = bi[1];
            top_idx[2 * s] = bi[0];
            top_idx[2 * s + 1] = bi[1];
            top_w[2 * s] = bw[0];
            top_w[2 * s + 1] = bw[1];
        }
    }
    __syncthreads();
    // counting sort of the pairs by expert, then token, then k: thread e owns expert e and walks the pairs in order
    const int npair = 2 * rows;
    if (tid < E) {
        int n = 0;
        for (int p = 0; p < npair; ++p) n += idx[p] == tid;
        cnt[tid] = n;
    }
    __syncthreads();
    if (tid == 0) {
        int o = 0;
        for (int e = 0; e < E; ++e) {
            off[e] = o;
            o += cnt[e];
        }
        off[E] = o;
    }
    __syncthreads();
    if (tid <= E) offsets[tid] = off[tid];
    if (tid < E) {
        int slot = off[tid];
        for (int p = 0; p < npair; ++p)
            if (idx[p] == tid) {
                slot_of[p] = slot;
                token_of[slot] = p >> 1;
                ++slot;
            }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void to_f32_kernel(const T* __restrict__ in, float* __restrict__ out, long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = to_f32<T>(in[i]);
}

// ---- the few-rows expert GEMM ----
template <typename T> struct M16;
template <> struct M16<bf16> {
    static __device__ __forceinline__ f32x4 mfma(typename H16<bf16>::vec a, typename H16<bf16>::vec b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
    }
};
template <> struct M16<f16> {
    static __device__ __forceinline__ f32x4 mfma(typename H16<f16>::vec a, typename H16<f16>::vec b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
    }
};

template <typename T>
__device__ __forceinline__ typename H16<T>::vec ld_frag(const T* __restrict__ p, bool ok) {
    uint4 v = make_uint4(0, 0, 0, 0);
    if (ok) v = *reinterpret_cast<const uint4*>(p);
    return __builtin_bit_cast(typename H16<T>::vec, v);
}

// BN output columns per workgroup (CT column tiles of 16), CH chunks of 16 slots per pass over K, U k-steps of 32 per batch
// of loads: (CH + CT) * U = 16 loads of 16 bytes per lane in flight before the first MFMA of a batch
constexpr int RG_BN = 32, RG_CT = RG_BN / 16, RG_CH = 2, RG_U = 4, RG_WAVES = 4;

template <typename T, int ACT, bool GATHER>
__global__ __launch_bounds__(256) void moe_rows_gemm_kernel(const T* __restrict__ A, const void* const* __restrict__ W,
                                                            const void* const* __restrict__ bias, T* __restrict__ C,
                                                            const int* __restrict__ offsets, const int* __restrict__ token_of,
                                                            int N, int K) {
    __shared__ float red[RG_WAVES][RG_CH * 16][RG_BN + 1];
    const int e = blockIdx.y;
    const int s0 = offsets[e], s1 = offsets[e + 1];
    if (s0 >= s1) return;  // (the whole workgroup: no barrier is left waiting)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, q = lane >> 4;
    const int n0 = blockIdx.x * RG_BN;
    const T* We = reinterpret_cast<const T*>(W[e]);
    const T* be = bias != nullptr ? reinterpret_cast<const T*>(bias[e]) : nullptr;
    // operand fragments of v_mfma_f32_16x16x32: lane (r, q) holds row r, k = 8q .. 8q+7 of the k-step, of A and of W alike
    const T* pb[RG_CT];
    bool okb[RG_CT];
#pragma unroll
    for (int ct = 0; ct < RG_CT; ++ct) {
        const int n = n0 + 16 * ct + r;
        okb[ct] = n < N;
        pb[ct] = We + (long long)(okb[ct] ? n : 0) * K + 8 * q;
    }
    const int nsteps = K / 32;  // (K % 64 == 0)
    for (int base = s0; base < s1; base += 16 * RG_CH) {
        const T* pa[RG_CH];
        bool oka[RG_CH];
#pragma unroll
        for (int c = 0; c < RG_CH; ++c) {
            const int slot = base + 16 * c + r;
            oka[c] = slot < s1;
            const int row = oka[c] ? (GATHER ? token_of[slot] : slot) : 0;
            pa[c] = A + (long long)row * K + 8 * q;
        }
        f32x4 acc[RG_CH][RG_CT];
#pragma unroll
        for (int c = 0; c < RG_CH; ++c)
#pragma unroll
            for (int ct = 0; ct < RG_CT; ++ct) acc[c][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
        // k-step s belongs to wave s % 4: the four waves read 256 contiguous bytes of every row together
        for (int st = wave; st < nsteps; st += RG_WAVES * RG_U) {
            typename H16<T>::vec fa[RG_U][RG_CH], fb[RG_U][RG_CT];
#pragma unroll
            for (int u = 0; u < RG_U; ++u) {
                const int s = st + RG_WAVES * u;
                const bool in = s < nsteps;
                const long long k = 32LL * s;
#pragma unroll
                for (int c = 0; c < RG_CH; ++c) fa[u][c] = ld_frag<T>(pa[c] + k, in && oka[c]);
#pragma unroll
                for (int ct = 0; ct < RG_CT; ++ct) fb[u][ct] = ld_frag<T>(pb[ct] + k, in && okb[ct]);
            }
#pragma unroll
            for (int u = 0; u < RG_U; ++u)
#pragma unroll
                for (int c = 0; c < RG_CH; ++c)
#pragma unroll
                    for (int ct = 0; ct < RG_CT; ++ct) acc[c][ct] = M16<T>::mfma(fa[u][c], fb[u][ct], acc[c][ct]);
        }
        // accumulator layout: lane (r, q) holds column r of rows 4q .. 4q+3
#pragma unroll
        for (int c = 0; c < RG_CH; ++c)
#pragma unroll
            for (int ct = 0; ct < RG_CT; ++ct)
#pragma unroll
                for (int i = 0; i < 4; ++i) red[wave][16 * c + 4 * q + i][16 * ct + r] = acc[c][ct][i];
        __syncthreads();
        // thread -> one slot, 8 consecutive columns
        if (tid < RG_CH * 16 * (RG_BN / 8)) {
            const int row = tid / (RG_BN / 8), c0 = (tid % (RG_BN / 8)) * 8;
            const int slot = base + row, gn = n0 + c0;
            if (slot < s1 && gn < N) {  // (N % 8 == 0: a chunk of 8 columns is inside or outside)
                float v[8];
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    v[j] = (red[0][row][c0 + j] + red[1][row][c0 + j]) + (red[2][row][c0 + j] + red[3][row][c0 + j]);
                if (be != nullptr) {
                    const Vec16<T> bv = load16<T>(be + gn);
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[j] += bv.get(j);
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = act_fwd_t<T>(ACT, v[j]);
                store16<T>(C + (long long)slot * N + gn, vec16_pack<T>(v));
            }
        }
        __syncthreads();  // (red is written again by the next pass)
    }
}

template <typename T, bool GATHER>
int launch_rows_gemm(const void* A, const void* const* W, const void* const* bias, void* C, const int* offsets, const int* token_of,
                     int E, int N, int K, int act, hipStream_t st) {
    const dim3 grid((unsigned)((N + RG_BN - 1) / RG_BN), (unsigned)E);
#define RG_L(ACT)                                                                                                            \
    moe_rows_gemm_kernel<T, ACT, GATHER><<<grid, 256, 0, st>>>((const T*)A, W, bias, (T*)C, offsets, token_of, N, K); \
    break
    switch (act) {
        case PK_ACT_NONE: RG_L(PK_ACT_NONE);
        case PK_ACT_RELU: RG_L(PK_ACT_RELU);
        case PK_ACT_GELU: RG_L(PK_ACT_GELU);
        case PK_ACT_GELU_TANH: RG_L(PK_ACT_GELU_TANH);
        case PK_ACT_SILU: RG_L(PK_ACT_SILU);
        default: PK_CHECK_ARG(false, "pk_moerows: activation %d", act);
    }
#undef RG_L
    PK_LAUNCH_CHECK();
    return 0;
}

int g_few_max = [] {
    const char* s = getenv("PK_MOE_ROWS_FEW_MAX");
    const int v = s != nullptr ? atoi(s) : 256;
    return v < 0 ? 0 : v;
}();

inline bool sizes_ok(long long rows, int E, int D, int F, int dtype) {
    return rows >= 1 && rows < (1LL << 29) && E >= 2 && E <= MOE_E_MAX && D >= 8 && F >= 8 && D % 8 == 0 && F % 8 == 0 &&
           D <= (1 << 19) && F <= (1 << 19) && (dtype == PK_F32 || dtype == PK_BF16 || dtype == PK_F16);
}

struct RowsScratch {
    char *logits, *xg, *h, *ys;
    float *logits32, *gate_value, *top_w, *prob_sum, *lb_coef, *lb_loss;
    int *top_idx, *offsets, *slot_of, *token_of, *top1_count;
    char* gate_ws;
    size_t gate_ws_bytes, total;
};
RowsScratch carve_rows(long long rows, int E, int D, int F, int dtype, bool few, char* base) {
    const size_t es = dtype == PK_F32 ? 4 : 2;
    RowsScratch s{};
    Carve c{base};
    s.logits = c.take((size_t)rows * E * es);
    s.top_idx = c.take<int>((size_t)rows * 2 * 4);
    s.top_w = c.take<float>((size_t)rows * 2 * 4);
    s.offsets = c.take<int>((size_t)(E + 1) * 4);
    s.slot_of = c.take<int>((size_t)rows * 2 * 4);
    s.token_of = c.take<int>((size_t)rows * 2 * 4);
    s.h = c.take((size_t)rows * 2 * F * es);
    s.ys = c.take((size_t)rows * 2 * D * es);
    if (!few) {
        s.logits32 = dtype == PK_F32 ? (float*)s.logits : c.take<float>((size_t)rows * E * 4);
        s.gate_value = c.take<float>((size_t)rows * E * 4);
        s.top1_count = c.take<int>((size_t)E * 4);
        s.prob_sum = c.take<float>((size_t)E * 4);
        s.lb_coef = c.take<float>((size_t)E * 4);
        s.lb_loss = c.take<float>(4);
        s.gate_ws_bytes = pk_moe_gate_scratch(rows, E);
        s.gate_ws = c.take(s.gate_ws_bytes);
        s.xg = c.take((size_t)rows * 2 * D * es);
    }
    s.total = c.total;
    return s;
}

}  // namespace

extern "C" {

int pk_moerows_few_max(int rows) {
    const int prev = g_few_max;
    if (rows >= 0) g_few_max = rows;
    return prev;
}

int pk_moerows_few(long long rows, int E, int D, int F, int dtype) {
    return sizes_ok(rows, E, D, F, dtype) && (dtype == PK_BF16 || dtype == PK_F16) && rows <= g_few_max &&
           rows <= PK_MOE_ROWS_MAX && D % 64 == 0 && F % 64 == 0;
}

size_t pk_moerows_scratch(long long rows, int E, int D, int F, int dtype) {
    if (!sizes_ok(rows, E, D, F, dtype)) return 0;
    // (both routes: the threshold may move between the query and the call)
    const size_t few = (dtype != PK_F32 && rows <= PK_MOE_ROWS_MAX) ? carve_rows(rows, E, D, F, dtype, true, nullptr).total : 0;
    const size_t grouped = carve_rows(rows, E, D, F, dtype, false, nullptr).total;
    return few > grouped ? few : grouped;
}

int pk_moerows_route(const void* logits, long long rows, int E, int dtype, int* top_idx, float* top_w, int* offsets,
                      int* slot_of, int* token_of, void* stream) {
    PK_CHECK_ARG(E >= 2 && E <= MOE_E_MAX, "pk_moerows_route: expert count %d outside [2, %d]", E, MOE_E_MAX);
    PK_CHECK_ARG(rows >= 1 && rows <= PK_MOE_ROWS_MAX, "pk_moerows_route: %lld rows outside [1, %d]", rows, PK_MOE_ROWS_MAX);
    PK_CHECK_ARG(logits && top_idx && top_w && offsets && slot_of && token_of, "pk_moerows_route: null logits or output");
    PK_DTYPE_SWITCH(dtype, "pk_moerows_route", {
        moe_route_rows_kernel<T><<<1, ROUTE_THREADS, 0, (hipStream_t)stream>>>((const T*)logits, (int)rows, E, top_idx, top_w, offsets,
                                                                               slot_of, token_of);
    })
    PK_LAUNCH_CHECK();
    return 0;
}

int pk_moerows(const void* x, void* y, const void* gate_w, const void* const* w1, const void* const* b1,
                const void* const* w2, const void* const* b2, long long rows, int E, int D, int F, int act, int dtype,
                void* scratch, size_t scratch_bytes, void* stream) {
    PK_CHECK_ARG(E >= 2 && E <= MOE_E_MAX, "pk_moerows: expert count %d outside [2, %d]", E, MOE_E_MAX);
    PK_CHECK_ARG(rows >= 1 && rows < (1LL << 29), "pk_moerows: row count %lld outside [1, 2^29)", rows);
    PK_CHECK_ARG(D >= 8 && F >= 8 && D % 8 == 0 && F % 8 == 0, "pk_moerows: D = %d, F = %d must be positive multiples of 8", D, F);
    PK_CHECK_ARG(D <= (1 << 19) && F <= (1 << 19), "pk_moerows: D = %d, F = %d beyond 2^19 columns", D, F);
    PK_CHECK_ARG(dtype == PK_F32 || dtype == PK_BF16 || dtype == PK_F16, "pk_moerows: dtype %d not supported", dtype);
    PK_CHECK_ARG(act >= PK_ACT_NONE && act <= PK_ACT_SILU, "pk_moerows: activation %d", act);
    PK_CHECK_ARG(x && y && gate_w && w1 && w2, "pk_moerows: null x / y / gate weight / pointer table");
    PK_CHECK_ARG((uintptr_t)x % 16 == 0 && (uintptr_t)y % 16 == 0, "pk_moerows: x and y must be 16-byte aligned");
    const size_t es = dtype == PK_F32 ? 4 : 2, span = (size_t)rows * D * es;
    PK_CHECK_ARG((const char*)y + span <= (const char*)x || (const char*)x + span <= (const char*)y, "pk_moerows: y overlaps x");
    const bool few = pk_moerows_few(rows, E, D, F, dtype) != 0;
    const size_t need = pk_moerows_scratch(rows, E, D, F, dtype);
    PK_CHECK_ARG(scratch && scratch_bytes >= need, "pk_moerows: scratch of %zu bytes, %zu needed", scratch ? scratch_bytes : 0, need);
    PK_CHECK_ARG((uintptr_t)scratch % 16 == 0, "pk_moerows: scratch must be 16-byte aligned");
    const RowsScratch s = carve_rows(rows, E, D, F, dtype, few, (char*)scratch);
    hipStream_t st = (hipStream_t)stream;
    // the gate's linear layer in the model's dtype: the pk_gemm call of functional.gemm(x2, wg) in MoEFn.forward
    int rc = pk_gemm(x, gate_w, s.logits, nullptr, nullptr, nullptr, rows, E, D, D, D, E, 0, 0, 0, 0, PK_ACT_NONE, 0, 1.f, dtype, 1,
                     nullptr, 0, nullptr, stream);
    if (rc != 0) return rc;
    if (few) {
        rc = pk_moerows_route(s.logits, rows, E, dtype, s.top_idx, s.top_w, s.offsets, s.slot_of, s.token_of, stream);
        if (rc != 0) return rc;
        if (dtype == PK_BF16) {
            rc = launch_rows_gemm<bf16, true>(x, w1, b1, s.h, s.offsets, s.token_of, E, F, D, act, st);
            if (rc == 0) rc = launch_rows_gemm<bf16, false>(s.h, w2, b2, s.ys, s.offsets, s.token_of, E, D, F, PK_ACT_NONE, st);
        } else {
            rc = launch_rows_gemm<f16, true>(x, w1, b1, s.h, s.offsets, s.token_of, E, F, D, act, st);
            if (rc == 0) rc = launch_rows_gemm<f16, false>(s.h, w2, b2, s.ys, s.offsets, s.token_of, E, D, F, PK_ACT_NONE, st);
        }
        if (rc != 0) return rc;
    } else {
        if (dtype != PK_F32) {  // `.float()`
            const long long n = rows * E;
            if (dtype == PK_BF16) to_f32_kernel<bf16><<<(unsigned)((n + 255) / 256), 256, 0, st>>>((const bf16*)s.logits, s.logits32, n);
            else to_f32_kernel<f16><<<(unsigned)((n + 255) / 256), 256, 0, st>>>((const f16*)s.logits, s.logits32, n);
            PK_LAUNCH_CHECK();
        }
        rc = pk_moe_gate(s.logits32, nullptr, rows, E, s.gate_value, s.top_idx, s.top_w, s.top1_count, s.prob_sum, s.lb_coef,
                         s.lb_loss, s.offsets, s.slot_of, s.token_of, s.gate_ws, s.gate_ws_bytes, stream);
        if (rc != 0) return rc;
        rc = pk_moe_gather(x, s.xg, s.token_of, s.offsets, s.slot_of, nullptr, rows, E, D, dtype, stream);
        if (rc != 0) return rc;
        rc = pk_moe_gemm(s.xg, w1, b1, s.h, nullptr, nullptr, s.offsets, 2 * rows, E, F, D, 0, act, 0, dtype, stream);
        if (rc != 0) return rc;
        rc = pk_moe_gemm(s.h, w2, b2, s.ys, nullptr, nullptr, s.offsets, 2 * rows, E, D, F, 0, PK_ACT_NONE, 0, dtype, stream);
        if (rc != 0) return rc;
    }
    return pk_moe_combine(s.ys, y, s.slot_of, s.top_w, rows, D, dtype, stream);
}

}  // extern "C"
