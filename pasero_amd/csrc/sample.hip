// Sampling search on the device: the choice of one token per sentence for one decoding step (pk_sample_select).
//
// Replaces, per step of pasero/decoding.py:1136-1190 (sample_on_the_fly): the repeat penalty's gather / where / scatter_,
// `.float().log_softmax(-1)`, the blacklist loop, the finished-row masked_fill_, and `argmax`, or `topk` + `exp` +
// `multinomial`, or `exp` + full descending `sort` + `cumsum` + mask + `multinomial`, and the forced prompt token.
//
//   pass 1  grid (chunks of V, rows), one WAVE per (row, chunk of 2048): the row scan of vocab_scan.h (chunk loader,
//           slot mapping, the chunk's (max, sum exp)) under the repeat penalty (rounded to the logits' dtype) and the
//           temperature; and the chunk's best live logit (for the greedy mode).
//   pass 2  one workgroup per row.  Folds the chunks into the row's log-sum-exp (fixed order, fp64).  greedy: the best of
//           the chunks' bests.  Otherwise NO sort: "first token, in the order (probability descending, id ascending),
//           whose inclusive cumulative weight exceeds a target" is a radix select over the 64-bit key
//           (bits of d = max - x) << 32 | id, ascending.  Level 0 is a 256-bucket histogram of floor(8 d) (buckets 1/8 nat
//           wide: live logits spread over them, where the raw exponent bits would pile them into two or three), kept in
//           LDS for both queries; every further level splits the crossing bucket's key range 256 ways with one more sweep
//           over the row, until at most 1024 keys remain: those are gathered into LDS and ranked exactly.
//           Query 1 (target: count k, or mass p) gives the kept set's size and mass M; query 2 (target u * M) the token.
//
// Mass is summed as 64-bit FIXED POINT (p * 2^62, exact for p >= 2^-39, truncated below) with integer LDS atomics:
// integer addition is associative, so every sum is independent of arrival order (two calls on the same inputs give the
// same bits) and carries no accumulation error at all — the only error left is expf's and the log-sum-exp's.
// Both launches are ordinary launches on the caller's stream; no global atomics, no inter-workgroup hand-off.
#include "vocab_scan.h"

namespace {

typedef unsigned long long u64;

constexpr int S1_WAVES = 4;            // pass 1: waves (= chunks) per workgroup
constexpr int S2_THREADS = 1024;
constexpr int S2_WAVES = S2_THREADS / 64;
constexpr int S_CAP = 1024;            // keys ranked exactly in LDS: one per thread
constexpr float FIX_ONE = 4611686018427387904.0f;  // 2^62
enum { MODE_GREEDY = 0, MODE_TOPK = 1, MODE_TOPP = 2, MODE_FULL = 3 };

struct SArgs {
    const void* logits;
    long long ld;
    int V, nchunks;
    const long long* hist;   // [rows][hist_ld], the first n_hist of every row
    long long hist_ld;
    int n_hist;
    float penalty, inv_temp;
    const long long* blacklist;
    int n_black;
    const unsigned char* finished;
    long long pad;
    float2* ms;   // [rows][nchunks]: chunk max, chunk sum of exp(x - max)
    u64* best;    // [rows][nchunks]: best live (logit, lowest id) of the chunk, 0 = none
    int mode, top_k;
    float top_p;
    const float* uniform_in;
    u64 seed, offset;
    const long long* forced;
    long long forced_stride;
    long long* token;
    long long token_stride;
    float *logprob, *lse;
    int* n_kept;
    float *kept_mass, *u_out;
};

template <typename T> __device__ __forceinline__ float penalised(float x, float penalty) {
    return to_f32(from_f32<T>(x < 0.f ? x * penalty : x / penalty));  // the reference works in the logits' dtype
}

// The (row, chunk)'s logits after repeat penalty and temperature, in vocab_scan.h's slots.  `dead`: bit s set = out of
// the row, blacklisted, or not `pad` on a finished row.
template <typename T, bool ALIGNED>
__device__ __forceinline__ void masked_chunk(const SArgs& a, int row, int chunk, int lane, float (&v)[SCAN_E], unsigned& dead) {
    const int base = chunk * SCAN_CHUNK;
    const int lim = a.V - base < SCAN_CHUNK ? a.V - base : SCAN_CHUNK;  // live tokens of the chunk
    load_chunk<T, ALIGNED>((const T*)a.logits + (long long)row * a.ld, a.V, base, lane, v, dead);
    if (a.n_hist > 0 && a.penalty != 1.0f) {
        unsigned pen = 0;  // a token that occurs twice in the history is penalised once
        const long long* h = a.hist + (long long)row * a.hist_ld;
        for (int i0 = 0; i0 < a.n_hist; i0 += 64) {
            const long long id = (i0 + lane < a.n_hist) ? h[i0 + lane] : -1;
            const int rel = (int)(id - base);
            u64 hits = __ballot(id >= base && id < (long long)base + lim);
            while (hits) {
                const int src = __ffsll((long long)hits) - 1;
                hits &= hits - 1;
                pen |= slot_bit<T>(__shfl(rel, src, 64), lane);
            }
        }
#pragma unroll
        for (int s = 0; s < SCAN_E; ++s)
            if ((pen >> s) & 1u) v[s] = penalised<T>(v[s], a.penalty);
    }
    if (a.inv_temp != 1.0f) {
#pragma unroll
        for (int s = 0; s < SCAN_E; ++s) v[s] *= a.inv_temp;
    }
    for (int b = 0; b < a.n_black; ++b) {
        const long long id = a.blacklist[b];
        if (id < base || id >= (long long)base + lim) continue;  // wave-uniform
        dead |= slot_bit<T>((int)(id - base), lane);
    }
    if (a.finished && a.finished[row]) {
        const long long r = a.pad - base;
        dead |= ~(r >= 0 && r < lim ? slot_bit<T>((int)r, lane) : 0u);
    }
}

template <typename T, bool ALIGNED>
__global__ __launch_bounds__(64 * S1_WAVES) void sample_pass1_kernel(SArgs a) {
    const int lane = threadIdx.x & 63;
    const int chunk = blockIdx.x * S1_WAVES + (threadIdx.x >> 6);
    const int row = blockIdx.y;
    if (chunk >= a.nchunks) return;  // wave-uniform
    float v[SCAN_E];
    unsigned dead;
    masked_chunk<T, ALIGNED>(a, row, chunk, lane, v, dead);
    // the normaliser covers the whole row: masked tokens do not leave it
    const float2 ms = chunk_max_sum(v);
    u64 key = 0;
    const int base = chunk * SCAN_CHUNK;
#pragma unroll
    for (int s = 0; s < SCAN_E; ++s) {
        if (!((dead >> s) & 1u) && v[s] > -INFINITY) {
            const u64 k = rank_key(v[s], (unsigned)slot_token<T>(base, lane, s));
            key = k > key ? k : key;
        }
    }
    key = wave_max_u64(key);
    if (lane == 0) {
        a.ms[(long long)row * a.nchunks + chunk] = ms;
        a.best[(long long)row * a.nchunks + chunk] = key;
    }
}

struct ScanOut {
    int found, bucket;
    unsigned n_in;        // keys in the crossing bucket
    u64 base_cnt, base_mass;  // found: count / mass in front of the crossing bucket; not found: the totals
};

// One wave: the first of 256 buckets whose inclusive cumulative weight (count or mass, on top of base_*) exceeds target.
__device__ __forceinline__ void scan256(const unsigned* cnt, const u64* mass, bool by_count, u64 target, u64 base_cnt,
                                        u64 base_mass, ScanOut* out, int lane) {
    u64 c[4], q[4], lc = 0, lq = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        c[i] = cnt[4 * lane + i];
        q[i] = mass[4 * lane + i];
        lc += c[i];
        lq += q[i];
    }
    u64 ic = lc, iq = lq;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const u64 tc = __shfl_up(ic, off, 64), tq = __shfl_up(iq, off, 64);
        if (lane >= off) {
            ic += tc;
            iq += tq;
        }
    }
    const u64 hits = __ballot((by_count ? base_cnt + ic : base_mass + iq) > target);
    if (!hits) {
        if (lane == 63) {
            out->found = 0;
            out->bucket = 0;
            out->n_in = 0;
            out->base_cnt = base_cnt + ic;
            out->base_mass = base_mass + iq;
        }
        return;
    }
    if (lane == __ffsll((long long)hits) - 1) {
        u64 ec = base_cnt + ic - lc, eq = base_mass + iq - lq;
        bool done = false;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (!done && (by_count ? ec + c[i] : eq + q[i]) > target) {
                out->found = 1;
                out->bucket = 4 * lane + i;
                out->n_in = (unsigned)c[i];
                out->base_cnt = ec;
                out->base_mass = eq;
                done = true;
            }
            ec += c[i];
            eq += q[i];
        }
    }
}

template <typename T, bool ALIGNED>
__global__ __launch_bounds__(S2_THREADS) void sample_pass2_kernel(SArgs a) {
    __shared__ unsigned h0c[256], hc[256];
    __shared__ u64 h0m[256], hm[256];
    __shared__ u64 cand_c[S_CAP], cand_q[S_CAP];
    __shared__ unsigned cand_n;
    __shared__ ScanOut sc;
    __shared__ struct { int found, token; u64 rank, mass; } res;
    __shared__ float s_max, s_logsum;
    __shared__ u64 wave_best[S2_WAVES];
    __shared__ int s_token;
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    // ---- the row's log-sum-exp from its chunks, in a fixed order ----
    if (wave == 0) {
        const float2 f = fold_chunks(a.ms + (long long)row * a.nchunks, a.nchunks, lane);
        if (lane == 0) {
            s_max = f.x;
            s_logsum = f.y;
        }
    }
    __syncthreads();
    const float m = s_max, logsum = s_logsum;

    // f(d, id) on every live token with a finite logit; d = max - x >= 0
    auto sweep = [&](auto&& f) {
        for (int c = wave; c < a.nchunks; c += S2_WAVES) {
            float v[SCAN_E];
            unsigned dead;
            masked_chunk<T, ALIGNED>(a, row, c, lane, v, dead);
#pragma unroll
            for (int s = 0; s < SCAN_E; ++s)
                if (!((dead >> s) & 1u) && v[s] > -INFINITY) f(m - v[s], slot_token<T>(c * SCAN_CHUNK, lane, s));
        }
    };
    auto fix = [&](float d) -> u64 { return __float2ull_rz(expf(-d - logsum) * FIX_ONE); };  // exp((x - max) - log(sum))
    auto key_of = [](float d, int id) -> u64 { return ((u64)__float_as_uint(d) << 32) | (u64)(unsigned)id; };

    // first token in the order whose inclusive cumulative count / mass exceeds `target` -> res
    auto query = [&](bool by_count, u64 target) {
        if (wave == 0) scan256(h0c, h0m, by_count, target, 0, 0, &sc, lane);
        __syncthreads();
        bool found = sc.found != 0;
        const int b0 = sc.bucket;
        u64 lo = (u64)__float_as_uint(b0 * 0.125f) << 32;
        u64 hi = b0 < 255 ? (u64)__float_as_uint((b0 + 1) * 0.125f) << 32 : (u64)0x7f800001u << 32;  // the last bucket is open-ended: d = inf included
        u64 bc = sc.base_cnt, bm = sc.base_mass;
        unsigned n_in = sc.n_in;
        __syncthreads();
        while (found && n_in > S_CAP) {
            const u64 R = hi - lo;
            const int sh = R <= 256 ? 0 : (64 - __clzll((long long)(R - 1))) - 8;
            for (int i = tid; i < 256; i += S2_THREADS) {
                hc[i] = 0;
                hm[i] = 0;
            }
            __syncthreads();
            sweep([&](float d, int id) {
                const u64 C = key_of(d, id);
                if (C >= lo && C < hi) {
                    const int dg = (int)((C - lo) >> sh);
                    atomicAdd(&hc[dg], 1u);
                    atomicAdd(&hm[dg], fix(d));
                }
            });
            __syncthreads();
            if (wave == 0) scan256(hc, hm, by_count, target, bc, bm, &sc, lane);
            __syncthreads();
            found = sc.found != 0;
            const u64 nlo = lo + ((u64)sc.bucket << sh), nhi = nlo + ((u64)1 << sh);
            lo = nlo;
            hi = nhi < hi ? nhi : hi;
            bc = sc.base_cnt;
            bm = sc.base_mass;
            n_in = sc.n_in;
            __syncthreads();
        }
        if (tid == 0) {
            cand_n = 0;
            res.found = 0;
            res.token = 0;
            res.rank = bc;   // not found: the totals
            res.mass = bm;
        }
        __syncthreads();
        if (found) {
            sweep([&](float d, int id) {
                const u64 C = key_of(d, id);
                if (C >= lo && C < hi) {
                    const unsigned slot = atomicAdd(&cand_n, 1u);
                    if (slot < S_CAP) {
                        cand_c[slot] = C;
                        cand_q[slot] = fix(d);
                    }
                }
            });
            __syncthreads();
            const int n = cand_n < S_CAP ? (int)cand_n : S_CAP;
            if (tid < n) {  // integer sums: the order the keys arrived in does not matter
                const u64 mine = cand_c[tid];
                u64 cc = 0, cq = 0;
                for (int j = 0; j < n; ++j) {
                    const bool in = cand_c[j] <= mine;
                    cc += in ? 1 : 0;
                    cq += in ? cand_q[j] : 0;
                }
                const u64 incl = by_count ? bc + cc : bm + cq;
                const u64 excl = by_count ? incl - 1 : incl - cand_q[tid];
                if (incl > target && excl <= target) {
                    res.found = 1;
                    res.token = (int)(unsigned)mine;
                    res.rank = bc + cc;
                    res.mass = bm + cq;
                }
            }
        }
        __syncthreads();
    };

    float u = 0.f;
    if (a.mode != MODE_GREEDY) {
        if (a.uniform_in) u = a.uniform_in[row];
        else u = (float)(philox4x32_10(a.seed, a.offset, (u64)row).x >> 8) * (1.0f / 16777216.0f);
    }
    int n_kept = 1;
    u64 M = 0;
    if (a.mode == MODE_GREEDY) {
        const u64* best = a.best + (long long)row * a.nchunks;
        u64 k = 0;
        for (int c = tid; c < a.nchunks; c += S2_THREADS) k = best[c] > k ? best[c] : k;
        k = wave_max_u64(k);
        if (lane == 0) wave_best[wave] = k;
        __syncthreads();
        if (tid == 0) {
            for (int i = 0; i < S2_WAVES; ++i) k = wave_best[i] > k ? wave_best[i] : k;
            s_token = k ? (int)key_index(k) : 0;  // nothing live: argmax of a row of -inf
        }
        __syncthreads();
    } else {
        for (int i = tid; i < 256; i += S2_THREADS) {
            h0c[i] = 0;
            h0m[i] = 0;
        }
        __syncthreads();
        sweep([&](float d, int id) {
            const float t = d * 8.0f;
            const int b = t >= 0.f && t < 255.f ? (int)t : 255;  // (a NaN from inf - inf lands in the last bucket too)
            atomicAdd(&h0c[b], 1u);
            atomicAdd(&h0m[b], fix(d));
        });
        __syncthreads();
        if (wave == 0) scan256(h0c, h0m, true, ~(u64)0, 0, 0, &sc, lane);  // crosses nowhere: the totals
        __syncthreads();
        const u64 tot_cnt = sc.base_cnt, tot_mass = sc.base_mass;
        __syncthreads();
        if (a.mode == MODE_TOPK) {
            query(true, (u64)(a.top_k - 1));
            n_kept = a.top_k;
            M = res.found ? res.mass : tot_mass;
        } else if (a.mode == MODE_TOPP) {
            query(false, (u64)((double)a.top_p * (double)FIX_ONE));
            n_kept = res.found ? (int)res.rank : a.V;  // every c_i <= p: the reference's mask is all true
            M = res.found ? res.mass : tot_mass;
        } else {
            n_kept = (int)tot_cnt;
            M = tot_mass;
        }
        __syncthreads();
        int tok = 0;
        if (M > 0) {
            u64 target = (u64)((double)u * (double)M);
            target = target < M ? target : M - 1;
            query(false, target);
            tok = res.token;
        }
        if (tid == 0) s_token = tok;
        __syncthreads();
    }

    // ---- forced token, the written token's masked log-probability, the outputs ----
    if (wave == 0) {
        long long tok = s_token;
        if (a.forced) {
            const long long f = a.forced[(long long)row * a.forced_stride];
            if (f != a.pad) tok = f;
        }
        float lp = -INFINITY;
        if (tok >= 0 && tok < a.V) {
            float x = to_f32(((const T*)a.logits + (long long)row * a.ld)[tok]) + 0.0f;
            bool masked = a.finished && a.finished[row] && tok != a.pad;
            bool seen = false;
            if (a.n_hist > 0 && a.penalty != 1.0f) {
                const long long* h = a.hist + (long long)row * a.hist_ld;
                for (int i = lane; i < a.n_hist; i += 64) seen |= h[i] == tok;
            }
            for (int b = lane; b < a.n_black; b += 64) masked |= a.blacklist[b] == tok;
            if (__ballot(seen)) x = penalised<T>(x, a.penalty);
            if (a.inv_temp != 1.0f) x *= a.inv_temp;
            if (!__ballot(masked)) lp = (x - m) - logsum;
        }
        if (lane == 0) {
            a.token[(long long)row * a.token_stride] = tok;
            a.logprob[row] = lp;
            a.lse[row] = m + logsum;
            a.n_kept[row] = n_kept;
            a.kept_mass[row] = a.mode == MODE_GREEDY ? 0.f : (float)((double)M / (double)FIX_ONE);
            a.u_out[row] = u;
        }
    }
}

}  // namespace

extern "C" size_t pk_sample_select_scratch(int B, long long V) {
    if (B <= 0 || V < 1 || V > (1LL << 27)) return 0;
    const size_t n = (size_t)B * n_chunks(V);
    return align256(n * sizeof(float2)) + align256(n * sizeof(u64));
}

extern "C" int pk_sample_select(const void* logits, long long ld, long long V, int B, int dtype, const long long* history,
                                long long history_ld, int n_hist, float penalty, float inv_temperature,
                                const long long* blacklist, int n_blacklist, const unsigned char* finished, long long pad,
                                int mode, int top_k, float top_p, const float* uniform_in, unsigned long long seed,
                                unsigned long long offset, const long long* forced, long long forced_stride, void* scratch,
                                size_t scratch_bytes, long long* token, long long token_stride, float* logprob, float* lse,
                                int* n_kept, float* kept_mass, float* u_out, void* stream) {
    PK_CHECK_ARG(V >= 1 && V <= (1LL << 27), "pk_sample_select: V %lld outside [1, 2^27]", V);
    PK_CHECK_ARG(ld >= V, "pk_sample_select: ld %lld < V %lld", ld, V);
    PK_CHECK_ARG(B >= 0 && B <= 65535, "pk_sample_select: B %d rows (at most 65535)", B);
    PK_CHECK_ARG(mode >= MODE_GREEDY && mode <= MODE_FULL, "pk_sample_select: mode %d", mode);
    PK_CHECK_ARG(!(top_k > 0 && top_p < 1.0f), "pk_sample_select: top_k %d and top_p %g together are not allowed", top_k,
                 (double)top_p);
    PK_CHECK_ARG(mode != MODE_TOPK || (top_k >= 1 && top_k <= V), "pk_sample_select: top_k %d outside [1, V]", top_k);
    PK_CHECK_ARG(mode != MODE_TOPP || (top_p > 0.0f && top_p < 1.0f), "pk_sample_select: top_p %g outside (0, 1)",
                 (double)top_p);
    PK_CHECK_ARG(n_blacklist >= 0 && (n_blacklist == 0 || blacklist), "pk_sample_select: blacklist");
    PK_CHECK_ARG(n_hist >= 0 && (n_hist == 0 || penalty == 1.0f || (history && history_ld >= n_hist)),
                 "pk_sample_select: history (n_hist %d, history_ld %lld)", n_hist, history_ld);
    PK_CHECK_ARG(penalty > 0.0f && inv_temperature > 0.0f, "pk_sample_select: penalty %g, inv_temperature %g",
                 (double)penalty, (double)inv_temperature);
    if (B == 0) return 0;
    PK_CHECK_ARG(logits && scratch && token && logprob && lse && n_kept && kept_mass && u_out,
                 "pk_sample_select: null argument");
    PK_CHECK_ARG(((uintptr_t)scratch & 255) == 0, "pk_sample_select: scratch must be 256-byte aligned");
    const size_t need = pk_sample_select_scratch(B, V);
    PK_CHECK_ARG(scratch_bytes >= need, "pk_sample_select: scratch %zu < %zu bytes", scratch_bytes, need);
    const int nc = n_chunks(V);
    SArgs a{};
    a.logits = logits; a.ld = ld; a.V = (int)V; a.nchunks = nc;
    a.hist = history; a.hist_ld = history_ld; a.n_hist = penalty == 1.0f ? 0 : n_hist;
    a.penalty = penalty; a.inv_temp = inv_temperature;
    a.blacklist = blacklist; a.n_black = n_blacklist; a.finished = finished; a.pad = pad;
    a.ms = (float2*)scratch;
    a.best = (u64*)((char*)scratch + align256((size_t)B * nc * sizeof(float2)));
    a.mode = mode; a.top_k = top_k; a.top_p = top_p; a.uniform_in = uniform_in; a.seed = seed; a.offset = offset;
    a.forced = forced; a.forced_stride = forced_stride; a.token = token; a.token_stride = token_stride;
    a.logprob = logprob; a.lse = lse; a.n_kept = n_kept; a.kept_mass = kept_mass; a.u_out = u_out;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid1((unsigned)((nc + S1_WAVES - 1) / S1_WAVES), (unsigned)B);
    PK_DTYPE_SWITCH(dtype, "pk_sample_select", {
        if (rows_aligned16(logits, ld, sizeof(T))) {
            hipLaunchKernelGGL((sample_pass1_kernel<T, true>), grid1, dim3(64 * S1_WAVES), 0, st, a);
            hipLaunchKernelGGL((sample_pass2_kernel<T, true>), dim3((unsigned)B), dim3(S2_THREADS), 0, st, a);
        } else {
            hipLaunchKernelGGL((sample_pass1_kernel<T, false>), grid1, dim3(64 * S1_WAVES), 0, st, a);
            hipLaunchKernelGGL((sample_pass2_kernel<T, false>), dim3((unsigned)B), dim3(S2_THREADS), 0, st, a);
        }
    })
    PK_LAUNCH_CHECK();
    return 0;
}
