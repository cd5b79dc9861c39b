// One bottleneck adapter on a handful of rows in ONE launch — the inference form of AdapterFn.forward
// (pasero/models/modules.py:248-370 AdapterLayer.forward):
//     y = x + s * ( act( LN(x) W_down^T + b_down ) W_up^T + b_up )          x, y [rows][d], W_down [p][d], W_up [d][p]
// A decoding step applies it after every layer (adapters.py:232-301) on 1 .. a few hundred rows: per-op it is three
// launches (LayerNorm, down-projection, up-projection) that each finish in a few microseconds of work, so the launches
// are the cost (gemm_skinny.hip's header: latency, not bandwidth — both weight matrices together are 2 d p elements,
// 256 KB at d = 1024, p = 64).
//
// The fused kernel (16-bit storage types): one workgroup of 4 waves = one tile of 32 rows x one slice of the d output
// columns.
//   1. LayerNorm: every wave normalises 8 rows in fp32 (statistics by wave butterflies, common.h), rounds to the
//      storage type and writes LN(x) to LDS — [32][d + 8] 16-bit, the whole tile (132 KB at d = 2048: a 16-bit tile fits
//      the 160 KiB of a CU, an fp32 copy would not).
//   2. down-projection on v_mfma_f32_32x32x16: the four waves split K = d in four and walk 32 (or 64) bottleneck columns
//      at a time, A fragments from LDS, W_down fragments straight from global memory in MFMA layout (16 B per lane, as
//      gemm_skinny.hip); the four partial tiles meet in LDS (fp32, fixed order), + bias, activation, rounded to the
//      storage type into the [32][p] bottleneck tile in LDS.
//   3. up-projection: each wave takes 32-column blocks of the slice, K = p, W_up fragments from global memory; epilogue
//      y = x + s * (acc + b_up), rounded once.
// Rounding to the storage type happens where the per-op path rounds: after LayerNorm, after the activation, at the output.
// Neither LN(x) nor the bottleneck activations touch global memory.
//
// Spreading the d columns: a tile alone is one workgroup per 32 rows — 2 of 256 CUs at 40 rows.  With `bps` 32-column
// blocks per slice the grid is (d / 32 / bps) x tiles; every slice repeats steps 1 and 2 (the down-projection is
// 32 x p x d, 1/ (d/32/bps) of which is "useful" — cheap next to an idle chip).  PK_ADAPTER_SLICE_BLOCKS (read at library
// load; 0 = one workgroup per tile) is the switch the measurement in docs/experiments.md was made with.
// y may alias x: then slices of one tile would race (one stores columns another still normalises), so an aliased call
// always runs one workgroup per tile, which has read all of its rows (step 1) before it stores any.
//
// Everything else (fp32, a d or p outside the fused range, PK_ADAPTER_FUSED=0) runs in the same C call as
// pk_residual_ln_fwd + pk_gemm + pk_gemm through a caller-provided scratch — the per-op launches, without Python.
#include <cstdlib>
#include "common.h"

namespace {

constexpr int AD_BM = 32, AD_WAVES = 4, AD_PAD = 8, AD_LDS_MAX = 160 * 1024;

struct AdapterArgs {
    const void *x, *ln_g, *ln_b, *wd, *bd, *wu, *bu;
    void* y;
    long long rows;
    int d, p, act, bps;
    float s, eps;
};

inline int p16_of(int p) { return (p + 15) / 16 * 16; }
inline size_t lds_bytes(int d, int p, int nbp) {
    return (size_t)AD_BM * (d + AD_PAD) * 2 + (size_t)AD_BM * (p16_of(p) + AD_PAD) * 2 +
           (size_t)AD_WAVES * AD_BM * (32 * nbp + 1) * 4;
}

template <typename T>
__device__ __forceinline__ typename H16<T>::vec as_frag(uint4 v) { return __builtin_bit_cast(typename H16<T>::vec, v); }

template <typename T, int NBP>
__global__ __launch_bounds__(256) void adapter_rows_kernel(AdapterArgs a) {
    extern __shared__ uint4 ad_smem[];
    const int d = a.d, p = a.p, P16 = (p + 15) / 16 * 16;
    const int HP = d + AD_PAD, AP = P16 + AD_PAD;
    constexpr int RP = 32 * NBP + 1;
    unsigned short* hs = reinterpret_cast<unsigned short*>(ad_smem);  // LN(x)            [32][HP]
    unsigned short* as = hs + AD_BM * HP;                             // act(down(LN(x))) [32][AP]
    float* red = reinterpret_cast<float*>(as + AD_BM * AP);           // K-split partials [4][32][RP]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const long long m0 = (long long)blockIdx.y * AD_BM;
    const T* x = reinterpret_cast<const T*>(a.x);  // (not __restrict__: y may be x)

    // ---- 1. LayerNorm of 8 rows per wave: all loads first, then the statistics row by row ----
    {
        uint4 xv[8][4];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const long long row = m0 + wave * 8 + i;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = (lane + 64 * j) * 8;
                xv[i][j] = make_uint4(0, 0, 0, 0);
                if (row < a.rows && c < d) xv[i][j] = *reinterpret_cast<const uint4*>(x + row * d + c);
            }
        }
        uint4 gv[4], bv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = (lane + 64 * j) * 8;
            gv[j] = bv[j] = make_uint4(0, 0, 0, 0);
            if (a.ln_g && c < d) gv[j] = *reinterpret_cast<const uint4*>(reinterpret_cast<const T*>(a.ln_g) + c);
            if (a.ln_g && a.ln_b && c < d) bv[j] = *reinterpret_cast<const uint4*>(reinterpret_cast<const T*>(a.ln_b) + c);
        }
        const float inv_d = 1.f / (float)d;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const bool live = m0 + wave * 8 + i < a.rows;
            float mean = 0.f, rstd = 1.f;
            if (a.ln_g) {  // (uniform over the workgroup: the butterflies below run with all 64 lanes)
                float sum = 0.f;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    Vec16<T> v;
                    v.raw = xv[i][j];
#pragma unroll
                    for (int e = 0; e < 8; ++e) sum += v.get(e);  // (chunks beyond d are zero)
                }
                mean = wave_sum(sum) * inv_d;
                float sq = 0.f;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if ((lane + 64 * j) * 8 < d) {
                        Vec16<T> v;
                        v.raw = xv[i][j];
#pragma unroll
                        for (int e = 0; e < 8; ++e) {
                            const float c = v.get(e) - mean;
                            sq += c * c;
                        }
                    }
                }
                rstd = rsqrtf(wave_sum(sq) * inv_d + a.eps);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = (lane + 64 * j) * 8;
                if (c >= d) continue;
                uint4 out = xv[i][j];  // no LayerNorm: the row itself
                if (a.ln_g) {
                    Vec16<T> v, g, b;
                    v.raw = xv[i][j];
                    g.raw = gv[j];
                    b.raw = bv[j];
                    float f[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) f[e] = (v.get(e) - mean) * rstd * g.get(e) + b.get(e);
                    out = vec16_pack<T>(f).raw;
                }
                if (!live) out = make_uint4(0, 0, 0, 0);
                *reinterpret_cast<uint4*>(hs + (wave * 8 + i) * HP + c) = out;
            }
        }
    }
    __syncthreads();

    // ---- 2. down-projection: K = d split over the four waves, NBP blocks of 32 bottleneck columns per pass ----
    {
        const T* __restrict__ wd = reinterpret_cast<const T*>(a.wd);
        const int kq = d / AD_WAVES, kb = wave * kq;  // d % 64 == 0: kq is a multiple of 16
        const unsigned short* ha = hs + r * HP + kb + 8 * h;
        for (int n0 = 0; n0 < P16; n0 += 32 * NBP) {
            f32x16 acc[NBP];
#pragma unroll
            for (int n = 0; n < NBP; ++n)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[n][i] = 0.f;
            constexpr int U = 4;
            for (int k = 0; k < kq; k += 16 * U) {
                uint4 fb[NBP][U], fa[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const bool in = k + 16 * u < kq;
#pragma unroll
                    for (int n = 0; n < NBP; ++n) {
                        const int col = n0 + 32 * n + r;
                        fb[n][u] = make_uint4(0, 0, 0, 0);
                        if (in && col < p) fb[n][u] = *reinterpret_cast<const uint4*>(wd + (long long)col * d + kb + 8 * h + k + 16 * u);
                    }
                    fa[u] = make_uint4(0, 0, 0, 0);
                    if (in) fa[u] = *reinterpret_cast<const uint4*>(ha + k + 16 * u);
                }
#pragma unroll
                for (int u = 0; u < U; ++u)
#pragma unroll
                    for (int n = 0; n < NBP; ++n) acc[n] = H16<T>::mfma(as_frag<T>(fa[u]), as_frag<T>(fb[n][u]), acc[n]);
            }
#pragma unroll
            for (int n = 0; n < NBP; ++n)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int row = (i & 3) + 8 * (i >> 2) + 4 * h;
                    red[(wave * AD_BM + row) * RP + 32 * n + r] = acc[n][i];
                }
            __syncthreads();
            for (int idx = tid; idx < AD_BM * 32 * NBP; idx += 256) {
                const int row = idx / (32 * NBP), cc = idx % (32 * NBP), col = n0 + cc;
                if (col >= P16) continue;
                unsigned short o = 0;  // columns [p, P16): the zero padding of the up-projection's last k-step
                if (col < p) {
                    float v = (red[(0 * AD_BM + row) * RP + cc] + red[(1 * AD_BM + row) * RP + cc]) +
                              (red[(2 * AD_BM + row) * RP + cc] + red[(3 * AD_BM + row) * RP + cc]);
                    if (a.bd) v += to_f32(reinterpret_cast<const T*>(a.bd)[col]);
                    o = H16<T>::bits(act_fwd_t<T>(a.act, v));
                }
                as[row * AP + col] = o;
            }
            __syncthreads();
        }
    }

    // ---- 3. up-projection: 32-column blocks of this workgroup's slice, one per wave at a time, K = p ----
    {
        const T* __restrict__ wu = reinterpret_cast<const T*>(a.wu);
        T* y = reinterpret_cast<T*>(a.y);
        const int nbt = d / 32;
        const int b0 = blockIdx.x * a.bps, b1 = min(b0 + a.bps, nbt);
        const unsigned short* pa = as + r * AP + 8 * h;
        for (int blk = b0 + wave; blk < b1; blk += AD_WAVES) {
            const int c0 = blk * 32;
            const T* pb = wu + (long long)(c0 + r) * p + 8 * h;
            f32x16 acc;
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] = 0.f;
            constexpr int U = 4;
            for (int k = 0; k < P16; k += 16 * U) {
                uint4 fa[U], fb[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int kk = k + 16 * u;
                    fa[u] = fb[u] = make_uint4(0, 0, 0, 0);
                    if (kk < P16) fa[u] = *reinterpret_cast<const uint4*>(pa + kk);
                    if (kk + 8 * h < p) fb[u] = *reinterpret_cast<const uint4*>(pb + kk);  // p % 8 == 0: a chunk is in or out
                }
#pragma unroll
                for (int u = 0; u < U; ++u) acc = H16<T>::mfma(as_frag<T>(fa[u]), as_frag<T>(fb[u]), acc);
            }
            const int col = c0 + r;
            const float sb = a.bu ? a.s * to_f32(reinterpret_cast<const T*>(a.bu)[col]) : 0.f;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const long long row = m0 + (i & 3) + 8 * (i >> 2) + 4 * h;
                if (row < a.rows) y[row * d + col] = from_f32<T>(to_f32(x[row * d + col]) + (a.s * acc[i] + sb));
            }
        }
    }
}

// PK_ADAPTER_FUSED=0: every call takes the three-launch route (the A/B switch of tools/adapter_decode_bench.py)
const bool g_fused_on = [] { const char* e = getenv("PK_ADAPTER_FUSED"); return !e || atoi(e) != 0; }();
// 32-column blocks per workgroup of the up-projection (0: one workgroup per tile); default 4 = one block per wave
const int g_slice_blocks = [] { const char* e = getenv("PK_ADAPTER_SLICE_BLOCKS"); return e ? atoi(e) : 4; }();

struct Fallback {
    char *h, *a, *sb;
    float *mean, *rstd;
    size_t total;
};
Fallback carve(long long rows, int d, int p, int dtype, char* base) {
    const size_t es = dtype == PK_F32 ? 4 : 2;
    Fallback f;
    Carve c{base};
    f.h = c.take((size_t)rows * d * es);
    f.a = c.take((size_t)rows * p * es);
    f.sb = c.take((size_t)d * es);
    f.mean = c.take<float>((size_t)rows * 4);
    f.rstd = c.take<float>((size_t)rows * 4);
    f.total = c.total;
    return f;
}

template <typename T, int NBP>
int launch_fused(const AdapterArgs& a, dim3 grid, size_t lds, hipStream_t st) {
    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&adapter_rows_kernel<T, NBP>),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, AD_LDS_MAX);
    if (attr != hipSuccess) {
        pk_set_error("pk_adapter_rows: hipFuncSetAttribute: %s", hipGetErrorString(attr));
        return (int)attr;
    }
    hipLaunchKernelGGL((adapter_rows_kernel<T, NBP>), grid, dim3(256), lds, st, a);
    PK_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" int pk_adapter_rows_fused(long long rows, int d, int p, int dtype) {
    (void)rows;
    return g_fused_on && (dtype == PK_BF16 || dtype == PK_F16) && d > 0 && d % 64 == 0 && d <= 2048 && p % 8 == 0 && p >= 8 &&
           p <= 512 && lds_bytes(d, p, 1) <= (size_t)AD_LDS_MAX;
}

extern "C" size_t pk_adapter_rows_scratch(long long rows, int d, int p, int dtype) {
    if (rows <= 0 || d <= 0 || p <= 0 || pk_adapter_rows_fused(rows, d, p, dtype)) return 0;
    return carve(rows, d, p, dtype, nullptr).total;
}

// The decoding step's own choice between the two routes (pk_adapter_step_fused; PK_ADAPTER_STEP_FUSED at library load).
// Default 0, by measurement (docs/experiments.md): inside the step the three launches are 0.09-0.14 ms per step faster
// than the fused kernel at the recipe's size.
int g_step_fused = [] { const char* e = getenv("PK_ADAPTER_STEP_FUSED"); return (e && atoi(e) != 0) ? 1 : 0; }();

extern "C" int pk_adapter_step_fused(int on) {
    const int prev = g_step_fused;
    if (on >= 0) g_step_fused = on != 0;
    return prev;
}

static int adapter_rows_impl(const void* x, void* y, const void* ln_g, const void* ln_b, const void* down_w,
                             const void* down_b, const void* up_w, const void* up_b, long long rows, int d, int p,
                             int act, float scaling, float eps, int dtype, void* scratch, size_t scratch_bytes,
                             void* stream, bool allow_fused);

extern "C" int pk_adapter_rows(const void* x, void* y, const void* ln_g, const void* ln_b, const void* down_w,
                               const void* down_b, const void* up_w, const void* up_b, long long rows, int d, int p,
                               int act, float scaling, float eps, int dtype, void* scratch, size_t scratch_bytes,
                               void* stream) {
    return adapter_rows_impl(x, y, ln_g, ln_b, down_w, down_b, up_w, up_b, rows, d, p, act, scaling, eps, dtype, scratch,
                             scratch_bytes, stream, true);
}

// for pk_decoder_step_ex (local to the library): the step's scratch always holds the three-launch need, so that
// pk_adapter_step_fused may change between two steps of one search
extern "C" size_t pk_adapter_rows_step_scratch(long long rows, int d, int p, int dtype) {
    return (rows <= 0 || d <= 0 || p <= 0) ? 0 : carve(rows, d, p, dtype, nullptr).total;
}
extern "C" int pk_adapter_rows_step(const void* x, void* y, const void* ln_g, const void* ln_b, const void* down_w,
                                    const void* down_b, const void* up_w, const void* up_b, long long rows, int d, int p,
                                    int act, float scaling, float eps, int dtype, void* scratch, size_t scratch_bytes,
                                    void* stream) {
    return adapter_rows_impl(x, y, ln_g, ln_b, down_w, down_b, up_w, up_b, rows, d, p, act, scaling, eps, dtype, scratch,
                             scratch_bytes, stream, g_step_fused != 0);
}

static int adapter_rows_impl(const void* x, void* y, const void* ln_g, const void* ln_b, const void* down_w,
                             const void* down_b, const void* up_w, const void* up_b, long long rows, int d, int p,
                             int act, float scaling, float eps, int dtype, void* scratch, size_t scratch_bytes,
                             void* stream, bool allow_fused) {
    PK_CHECK_ARG(x && y && down_w && up_w, "pk_adapter_rows: null argument");
    PK_CHECK_ARG(rows >= 0 && d > 0 && p > 0, "pk_adapter_rows: bad sizes (rows=%lld d=%d p=%d)", rows, d, p);
    PK_CHECK_ARG(dtype == PK_F32 || dtype == PK_BF16 || dtype == PK_F16, "pk_adapter_rows: dtype %d not supported", dtype);
    PK_CHECK_ARG(act >= PK_ACT_NONE && act <= PK_ACT_SILU, "pk_adapter_rows: bad activation %d", act);
    const size_t es = dtype == PK_F32 ? 4 : 2, bytes = (size_t)rows * d * es;
    const uintptr_t xa = (uintptr_t)x, ya = (uintptr_t)y;
    PK_CHECK_ARG(xa == ya || xa + bytes <= ya || ya + bytes <= xa, "pk_adapter_rows: y must be x itself or not overlap it");
    const bool fused = allow_fused && pk_adapter_rows_fused(rows, d, p, dtype);
    if (!fused) {
        const size_t need = carve(rows, d, p, dtype, nullptr).total;
        PK_CHECK_ARG(rows == 0 || (scratch && scratch_bytes >= need), "pk_adapter_rows: scratch too small (%zu < %zu)",
                     scratch ? scratch_bytes : (size_t)0, need);
    } else {
        PK_CHECK_ARG(((xa | ya | (uintptr_t)ln_g | (uintptr_t)ln_b | (uintptr_t)down_w | (uintptr_t)up_w) % 16) == 0,
                     "pk_adapter_rows: operands of the fused kernel must be 16-byte aligned");
    }
    if (rows == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    if (fused) {
        AdapterArgs a{x, ln_g, ln_b, down_w, down_b, up_w, up_b, y, rows, d, p, act, 0, scaling, eps};
        const long long tiles = (rows + AD_BM - 1) / AD_BM;
        PK_CHECK_ARG(tiles <= 65535, "pk_adapter_rows: too many rows (%lld)", rows);
        const int nbt = d / 32;
        // slices only where they buy parallelism (few tiles) and cannot race (y is not x)
        a.bps = (xa == ya || g_slice_blocks <= 0 || tiles >= 64) ? nbt : (g_slice_blocks < nbt ? g_slice_blocks : nbt);
        dim3 grid((unsigned)((nbt + a.bps - 1) / a.bps), (unsigned)tiles);
        const bool two = p > 32 && lds_bytes(d, p, 2) <= (size_t)AD_LDS_MAX;
        const size_t lds = lds_bytes(d, p, two ? 2 : 1);
        if (dtype == PK_BF16) return two ? launch_fused<bf16, 2>(a, grid, lds, st) : launch_fused<bf16, 1>(a, grid, lds, st);
        return two ? launch_fused<f16, 2>(a, grid, lds, st) : launch_fused<f16, 1>(a, grid, lds, st);
    }
    // the per-op sequence (autograd.AdapterFn.forward): LayerNorm, down-projection + activation, up-projection with the
    // scale and the residual in its epilogue ((v + b) s = s v + s b: the bias is scaled first)
    Fallback f = carve(rows, d, p, dtype, (char*)scratch);
    const void* hin = x;
    int rc;
    if (ln_g) {
        rc = pk_residual_ln_fwd(x, nullptr, ln_g, ln_b, nullptr, f.h, f.mean, f.rstd, rows, d, eps, 0.f, 0, 0, dtype, stream);
        if (rc != 0) return rc;
        hin = f.h;
    }
    rc = pk_gemm(hin, down_w, f.a, down_b, nullptr, nullptr, rows, p, d, d, d, p, 0, 0, 0, 0, act, 0, 1.f, dtype, 1, nullptr, 0,
                 nullptr, stream);
    if (rc != 0) return rc;
    const void* ub = up_b;
    if (up_b && scaling != 1.f) {
        rc = pk_scale(up_b, f.sb, d, nullptr, scaling, dtype, stream);
        if (rc != 0) return rc;
        ub = f.sb;
    }
    return pk_gemm(f.a, up_w, y, ub, x, nullptr, rows, d, p, p, p, d, d, 0, 0, 0, PK_ACT_NONE, 1, scaling, dtype, 1, nullptr, 0,
                   nullptr, stream);
}
