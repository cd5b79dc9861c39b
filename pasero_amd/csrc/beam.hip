// Beam search on the device: the selection of one search step for a whole batch (pk_beam_select) and the re-ordering
// of the native decoding step's self-attention caches by the chosen beams (pk_beam_reorder).
//
// Replaces, per step of pasero/decoding.py:1225-1657 (beam_search): `.float().log_softmax(-1)`, the blacklist and
// forced-token masking, `scores += hyp_scores`, `topk(2K)` over (B, K*V), the EOS mask and the second
// `topk(beam_range + eos_mask * 2K, largest=False)` (:1391-1449, :1539-1549); and, for the caches of the native step,
// `Decoder.reorder_state` (pasero/models/transformer.py:68-75).
//
// pk_beam_select reads the logits once, in their own dtype:
//   pass 1  grid (chunks of V, rows), one WAVE per (row, chunk of 2048): the row scan of vocab_scan.h (chunk loader,
//           slot mapping, the chunk's (max, sum exp)) and the chunk's top 2K RAW logits — log_softmax is
//           monotone within a row and no (row, chunk) can own more than 2K of a sentence's 2K winners.  The top 2K are
//           taken by 2K rounds of a wave-wide arg-max over each lane's cached best; only the winning lane rescans.
//   pass 2  one workgroup per sentence: folds the chunks' (max, sum) into each row's log-sum-exp, rescores the
//           rows * chunks * 2K survivors with the reference's fp32 arithmetic ((x - max) - log(sum) + bias + hyp), sorts
//           the best 2K by (score descending, flat index k*V + v ascending — the order of a stable descending sort),
//           applies the EOS rule and writes the outputs.
// Both are ordinary launches on the caller's stream; no atomics, no inter-workgroup hand-off inside a launch.
//
// Known corner: pass 1 ranks by the raw logit, pass 2 by the rounded fp32 score.  Two DIFFERENT logits of one row whose
// scores round to the same float are ranked by index in pass 2; if such a pair straddles position 2K of its own
// (row, chunk) the one pass 1 dropped cannot come back.  Equal logits (the ties 16-bit inputs produce) are exact.
#include "vocab_scan.h"

namespace {

constexpr int BEAM_MAX_K = 16;
constexpr int P1_WAVES = 4;            // waves (= chunks) per workgroup
constexpr int P2_THREADS = 1024;
constexpr int REORDER_MAX_LAYERS = 48;

struct P1Args {
    const void* logits;
    long long ld;
    int V, K, first_step, nchunks;
    const long long* forced;
    long long pad, eos;
    const long long* blacklist;
    int n_black;
    float2* ms;      // [rows][nchunks]: chunk max, chunk sum of exp(x - max)
    float* cand_x;   // [rows][nchunks][2K] raw logit
    int* cand_i;     // [rows][nchunks][2K] token id
};

template <typename T, bool ALIGNED>
__global__ __launch_bounds__(64 * P1_WAVES) void beam_pass1_kernel(P1Args a) {
    const int lane = threadIdx.x & 63;
    const int chunk = blockIdx.x * P1_WAVES + (threadIdx.x >> 6);
    const int row = blockIdx.y;
    if (chunk >= a.nchunks) return;                     // wave-uniform
    if (a.first_step && (row % a.K) != 0) return;       // scores[::beam_size] (decoding.py:1423-1425)
    const int R = 2 * a.K;
    const T* p = (const T*)a.logits + (long long)row * a.ld;
    const int base = chunk * SCAN_CHUNK;
    float v[SCAN_E];
    unsigned gone;
    load_chunk<T, ALIGNED>(p, a.V, base, lane, v, gone);  // bit s: slot s is out of the row or already taken

    // ---- the chunk's share of the row's softmax: (max, sum exp(x - max)) over the unmasked logits ----
    const float2 ms = chunk_max_sum(v);
    if (lane == 0) a.ms[(long long)row * a.nchunks + chunk] = ms;

    // ---- what may not be chosen: blacklisted ids, and on a forced row everything but the forced token ----
    if (a.forced) {
        const long long f = a.forced[row];
        if (f != a.pad && f != a.eos) {
#pragma unroll
            for (int s = 0; s < SCAN_E; ++s)
                if (slot_token<T>(base, lane, s) != f) v[s] = -INFINITY;
        }
    }
    for (int b = 0; b < a.n_black; ++b) {
        const long long id = a.blacklist[b];
        if (id < base || id >= (long long)base + SCAN_CHUNK) continue;  // wave-uniform
        const unsigned hit = slot_bit<T>((int)(id - base), lane);
#pragma unroll
        for (int s = 0; s < SCAN_E; ++s)
            if ((hit >> s) & 1u) v[s] = -INFINITY;
    }

    // ---- top 2K of the chunk: 2K rounds of a wave-wide arg-max over each lane's best; lane r keeps winner r ----
    float bv;
    int bs;
    auto rescan = [&]() {
        bv = -INFINITY;
        bs = -1;
#pragma unroll
        for (int s = 0; s < SCAN_E; ++s) {
            const bool live = !((gone >> s) & 1u);
            if (live && (bs < 0 || v[s] > bv)) { bv = v[s]; bs = s; }
        }
    };
    rescan();
    float out_x = -INFINITY;
    int out_i = 0;
    for (int r = 0; r < R; ++r) {
        unsigned long long key = 0;
        if (bs >= 0) key = rank_key(bv, (unsigned)slot_token<T>(0, lane, bs));
        const unsigned long long w = wave_max_u64(key);
        if (w != 0) {
            if (lane == r) {
                out_x = key_score(w);
                out_i = base + (int)key_index(w);
            }
            if (key == w) {  // one lane: the index is part of the key
                gone |= 1u << bs;
                rescan();
            }
        }
    }
    if (lane < R) {
        const long long o = ((long long)row * a.nchunks + chunk) * R + lane;
        a.cand_x[o] = out_x;
        a.cand_i[o] = out_i;
    }
}

struct P2Args {
    int V, K, first_step, nchunks;
    long long eos;
    const float2* ms;
    const float* cand_x;
    const int* cand_i;
    unsigned long long* keys;  // [B][K * nchunks * 2K]
    const float* hyp_in;
    const float* row_bias;
    const unsigned char* eos_counts;
    float* cand_score;
    int *cand_beam, *cand_tok, *cand_eos, *n_eos;
    long long *sel_beam, *sel_tok;
    float *sel_score, *lse_out;
};

__global__ __launch_bounds__(P2_THREADS) void beam_pass2_kernel(P2Args a) {
    __shared__ float row_max[BEAM_MAX_K], row_logsum[BEAM_MAX_K];
    __shared__ unsigned long long wave_best[2][P2_THREADS / 64];
    __shared__ unsigned long long sorted[2 * BEAM_MAX_K];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = a.K, R = 2 * K, nrows = a.first_step ? 1 : K;

    // ---- each row's log-sum-exp from its chunks ----
    for (int k = wave; k < nrows; k += P2_THREADS / 64) {
        const float2 f = fold_chunks(a.ms + (long long)(b * K + k) * a.nchunks, a.nchunks, lane);
        if (lane == 0) {
            row_max[k] = f.x;
            row_logsum[k] = f.y;
            if (a.lse_out) a.lse_out[b * K + k] = f.x + f.y;
        }
    }
    __syncthreads();

    // ---- score the survivors: ((x - max) - log(sum)) + bias + hyp, fp32, in the reference's order ----
    const int per_row = a.nchunks * R, N = nrows * per_row;
    unsigned long long* keys = a.keys + (long long)b * K * per_row;
    for (int c = tid; c < N; c += P2_THREADS) {
        const int k = c / per_row, row = b * K + k;
        const long long src = (long long)row * per_row + (c - k * per_row);
        float s = (a.cand_x[src] - row_max[k]) - row_logsum[k];
        if (a.row_bias) s += a.row_bias[row];
        if (a.hyp_in) s += a.hyp_in[row];
        keys[c] = rank_key(s, (unsigned)k * (unsigned)a.V + (unsigned)a.cand_i[src]);
    }
    __syncthreads();  // a thread rescans only its own keys, but keep the phases apart

    // ---- the best 2K, in order: round r takes the largest key below round r-1's ----
    unsigned long long prev = ~0ull, mine = 0;
    auto rescan = [&]() {
        mine = 0;
        for (int c = tid; c < N; c += P2_THREADS) {
            const unsigned long long k = keys[c];
            if (k < prev && k > mine) mine = k;
        }
    };
    rescan();
    for (int r = 0; r < R; ++r) {
        const unsigned long long w = wave_max_u64(mine);
        if (lane == 0) wave_best[r & 1][wave] = w;
        __syncthreads();
        unsigned long long best = 0;
#pragma unroll
        for (int i = 0; i < P2_THREADS / 64; ++i) {
            const unsigned long long o = wave_best[r & 1][i];
            best = o > best ? o : best;
        }
        if (tid == 0) sorted[r] = best;
        prev = best;
        if (best == 0) {
            mine = 0;
        } else if (mine == best) {
            rescan();
        }
    }
    __syncthreads();

    // ---- EOS rule and the K continued beams (2K <= 32 records: one thread) ----
    if (tid == 0) {
        const bool counts = a.eos_counts ? a.eos_counts[b] != 0 : true;
        int n_eos = 0, nsel = 0;
        for (int r = 0; r < R; ++r) {
            const unsigned long long w = sorted[r];
            float score = -INFINITY;
            int k = 0, tok = 0;
            if (w != 0) {
                score = key_score(w);
                const unsigned flat = key_index(w);
                k = (int)(flat / (unsigned)a.V);
                tok = (int)(flat % (unsigned)a.V);
            }
            const bool is_eos = tok == a.eos && isfinite(score) && counts;
            const int o = b * R + r;
            a.cand_score[o] = score;
            a.cand_beam[o] = k;
            a.cand_tok[o] = tok;
            a.cand_eos[o] = is_eos ? 1 : 0;
            if (is_eos && r < K) ++n_eos;
            if (!is_eos && nsel < K) {
                a.sel_beam[b * K + nsel] = (long long)b * K + k;
                a.sel_tok[b * K + nsel] = tok;
                a.sel_score[b * K + nsel] = score;
                ++nsel;
            }
        }
        for (; nsel < K; ++nsel) {  // cannot happen (a beam has one EOS): keep the outputs defined
            a.sel_beam[b * K + nsel] = (long long)b * K;
            a.sel_tok[b * K + nsel] = 0;
            a.sel_score[b * K + nsel] = -INFINITY;
        }
        a.n_eos[b] = n_eos;
    }
}

struct ReorderArgs {
    const void* src[2 * REORDER_MAX_LAYERS];
    void* dst[2 * REORDER_MAX_LAYERS];
};

// dst[l][r][0:t][:] = src[l][sel[r]][0:t][:]; the first t rows of a cache line are contiguous: t * d elements
__global__ __launch_bounds__(256) void beam_reorder_kernel(ReorderArgs a, const long long* __restrict__ sel, int rows_in,
                                                           long long row_bytes, long long copy_bytes) {
    const long long s = sel[blockIdx.x];
    if (s < 0 || s >= rows_in) return;
    const char* src = (const char*)a.src[blockIdx.y] + s * row_bytes;
    char* dst = (char*)a.dst[blockIdx.y] + (long long)blockIdx.x * row_bytes;
    for (long long o = (long long)threadIdx.x * 16; o < copy_bytes; o += 256 * 16)
        *reinterpret_cast<uint4*>(dst + o) = *reinterpret_cast<const uint4*>(src + o);
}

struct Scratch {
    float2* ms;
    float* cand_x;
    int* cand_i;
    unsigned long long* keys;
    size_t total;
};
Scratch carve(int B, int K, long long V, char* base) {
    const size_t rows = (size_t)B * K, nc = n_chunks(V), R = 2 * (size_t)K;
    Carve c{base};
    Scratch s;
    s.ms = c.take<float2>(rows * nc * sizeof(float2));
    s.cand_x = c.take<float>(rows * nc * R * sizeof(float));
    s.cand_i = c.take<int>(rows * nc * R * sizeof(int));
    s.keys = c.take<unsigned long long>(rows * nc * R * sizeof(unsigned long long));
    s.total = c.total;
    return s;
}

}  // namespace

extern "C" size_t pk_beam_select_scratch(int B, int K, long long V) {
    if (B <= 0 || K < 1 || K > BEAM_MAX_K || V < 1) return 0;
    return carve(B, K, V, nullptr).total;
}

extern "C" int pk_beam_select(const void* logits, long long ld, long long V, int B, int K, int dtype, const float* hyp_in,
                              const float* row_bias, const long long* forced, long long pad, long long eos,
                              const long long* blacklist, int n_blacklist, const unsigned char* eos_counts, void* scratch,
                              size_t scratch_bytes, float* cand_score, int* cand_beam, int* cand_tok, int* cand_eos,
                              int* n_eos, long long* sel_beam, long long* sel_tok, float* sel_score, float* lse_out,
                              void* stream) {
    PK_CHECK_ARG(K >= 1 && K <= BEAM_MAX_K, "pk_beam_select: beam size %d outside [1, %d]", K, BEAM_MAX_K);
    PK_CHECK_ARG(B >= 0 && (long long)B * K <= 65535, "pk_beam_select: B * K = %lld rows (at most 65535)", (long long)B * K);
    PK_CHECK_ARG(V >= 1 && V <= (1LL << 27) && ld >= V, "pk_beam_select: V %lld, ld %lld", V, ld);
    PK_CHECK_ARG(n_blacklist >= 0 && (n_blacklist == 0 || blacklist), "pk_beam_select: blacklist");
    if (B == 0) return 0;
    PK_CHECK_ARG(logits && scratch && cand_score && cand_beam && cand_tok && cand_eos && n_eos && sel_beam && sel_tok &&
                     sel_score, "pk_beam_select: null argument");
    PK_CHECK_ARG(((uintptr_t)scratch & 255) == 0, "pk_beam_select: scratch must be 256-byte aligned");
    Scratch s = carve(B, K, V, (char*)scratch);
    PK_CHECK_ARG(scratch_bytes >= s.total, "pk_beam_select: scratch %zu < %zu bytes", scratch_bytes, s.total);
    hipStream_t st = (hipStream_t)stream;
    const int nc = n_chunks(V);
    P1Args a1{logits, ld, (int)V, K, hyp_in == nullptr, nc, forced, pad, eos, blacklist, n_blacklist, s.ms, s.cand_x, s.cand_i};
    const dim3 grid1((unsigned)((nc + P1_WAVES - 1) / P1_WAVES), (unsigned)(B * K));
    PK_DTYPE_SWITCH(dtype, "pk_beam_select", {
        if (rows_aligned16(logits, ld, sizeof(T))) hipLaunchKernelGGL((beam_pass1_kernel<T, true>), grid1, dim3(64 * P1_WAVES), 0, st, a1);
        else hipLaunchKernelGGL((beam_pass1_kernel<T, false>), grid1, dim3(64 * P1_WAVES), 0, st, a1);
    })
    PK_LAUNCH_CHECK();
    P2Args a2{(int)V, K, hyp_in == nullptr, nc, eos, s.ms, s.cand_x, s.cand_i, s.keys, hyp_in, row_bias, eos_counts,
              cand_score, cand_beam, cand_tok, cand_eos, n_eos, sel_beam, sel_tok, sel_score, lse_out};
    hipLaunchKernelGGL(beam_pass2_kernel, dim3((unsigned)B), dim3(P2_THREADS), 0, st, a2);
    PK_LAUNCH_CHECK();
    return 0;
}

extern "C" int pk_beam_reorder(const void* const* src_k, const void* const* src_v, void* const* dst_k, void* const* dst_v,
                               int n_layers, const long long* sel_beam, int rows_out, int rows_in, int t, long long cap,
                               int d, int dtype, void* stream) {
    PK_CHECK_ARG(src_k && src_v && dst_k && dst_v && n_layers >= 1, "pk_beam_reorder: null table");
    PK_CHECK_ARG(rows_out >= 0 && rows_out <= 65535 && rows_in >= 1 && t >= 0 && t <= cap && d >= 1,
                 "pk_beam_reorder: rows_out %d rows_in %d t %d cap %lld d %d", rows_out, rows_in, t, cap, d);
    PK_CHECK_ARG(dtype == PK_F32 || dtype == PK_BF16 || dtype == PK_F16, "pk_beam_reorder: dtype %d not supported", dtype);
    const long long es = dtype == PK_F32 ? 4 : 2;
    PK_CHECK_ARG(((long long)d * es) % 16 == 0, "pk_beam_reorder: a cache row of %d elements is not a multiple of 16 bytes", d);
    if (rows_out == 0 || t == 0) return 0;
    PK_CHECK_ARG(sel_beam, "pk_beam_reorder: null indices");
    for (int l = 0; l < n_layers; ++l) {
        PK_CHECK_ARG(src_k[l] && src_v[l] && dst_k[l] && dst_v[l], "pk_beam_reorder: null buffer (layer %d)", l);
        PK_CHECK_ARG(src_k[l] != dst_k[l] && src_v[l] != dst_v[l], "pk_beam_reorder: an in-place gather races (layer %d)", l);
        PK_CHECK_ARG(((uintptr_t)src_k[l] | (uintptr_t)src_v[l] | (uintptr_t)dst_k[l] | (uintptr_t)dst_v[l]) % 16 == 0,
                     "pk_beam_reorder: buffers must be 16-byte aligned (layer %d)", l);
    }
    hipStream_t st = (hipStream_t)stream;
    for (int l0 = 0; l0 < n_layers; l0 += REORDER_MAX_LAYERS) {  // one launch up to 48 layers
        const int n = n_layers - l0 < REORDER_MAX_LAYERS ? n_layers - l0 : REORDER_MAX_LAYERS;
        ReorderArgs a;
        for (int l = 0; l < n; ++l) {
            a.src[2 * l] = src_k[l0 + l];
            a.src[2 * l + 1] = src_v[l0 + l];
            a.dst[2 * l] = dst_k[l0 + l];
            a.dst[2 * l + 1] = dst_v[l0 + l];
        }
        hipLaunchKernelGGL(beam_reorder_kernel, dim3((unsigned)rows_out, (unsigned)(2 * n)), dim3(256), 0, st, a, sel_beam,
                           rows_in, cap * d * es, (long long)t * d * es);
        PK_LAUNCH_CHECK();
    }
    return 0;
}
