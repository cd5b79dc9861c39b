// The scan of one vocabulary row shared by the selection kernels (beam.hip, sample.hip): a row of V logits is cut into
// chunks of 2048, one WAVE per (row, chunk) holds its chunk in registers (16-byte loads, the operand is used once: no
// LDS) and reduces it to (max, sum exp); one wave later folds a row's chunks into its log-sum-exp.  Also the 64-bit rank
// key both kernels order candidates by.  Everything lives in an anonymous namespace (one copy per translation unit).
// The floating-point operations and their order are part of the kernels' contract (bit-for-bit repeatable results).
#pragma once
#include <math.h>
#include "common.h"

namespace {

constexpr int SCAN_E = 32;               // logits per lane
constexpr int SCAN_CHUNK = 64 * SCAN_E;  // logits per wave
inline int n_chunks(long long V) { return (int)((V + SCAN_CHUNK - 1) / SCAN_CHUNK); }
// 16-byte loads need every row to start on a 16-byte boundary; anything else is read element by element
inline bool rows_aligned16(const void* p, long long ld, size_t elem_bytes) {
    return ((uintptr_t)p % 16 == 0) && ((ld * (long long)elem_bytes) % 16 == 0);
}

// float -> unsigned whose integer order is the float order (-inf lowest); +0 and -0 are made one value first
__device__ __forceinline__ unsigned ordered_bits(float f) {
    unsigned u = __float_as_uint(f + 0.0f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ordered_float(unsigned o) {
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}
// larger key = better candidate: score first, then the LOWER index; 0 = no candidate
__device__ __forceinline__ unsigned long long rank_key(float score, unsigned index) {
    return ((unsigned long long)ordered_bits(score) << 32) | (unsigned long long)(0xffffffffu - index);
}
__device__ __forceinline__ float key_score(unsigned long long k) { return ordered_float((unsigned)(k >> 32)); }
__device__ __forceinline__ unsigned key_index(unsigned long long k) { return 0xffffffffu - (unsigned)k; }
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long k) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        unsigned long long o = __shfl_xor(k, off, 64);
        k = o > k ? o : k;
    }
    return k;
}

// Register slot s = j * EPV + e of a lane holds token base + (j * 64 + lane) * EPV + e (EPV elements per 16 bytes):
// ascending in s within a lane, and a wave's j-th load covers 64 * EPV consecutive tokens.
template <typename T> __device__ __forceinline__ int slot_token(int base, int lane, int s) {
    constexpr int EPV = 16 / sizeof(T);
    return base + ((s / EPV) * 64 + lane) * EPV + (s % EPV);
}
// the inverse, as a mask: bit s set in the one lane whose slot s holds token base + rel (0 <= rel < SCAN_CHUNK), else 0
template <typename T> __device__ __forceinline__ unsigned slot_bit(int rel, int lane) {
    constexpr int EPV = 16 / sizeof(T);
    return lane == (rel / EPV) % 64 ? 1u << ((rel / (64 * EPV)) * EPV + rel % EPV) : 0u;
}

// v[s] = the logit of slot s of the chunk that starts at token `base` of the row `p` (-inf out of the row); `out`: bit s
// set = slot s is out of the row.  Nothing past element V - 1 is read: the vector that straddles the row's end is read
// by element.  (`out` is written in place and takes one closed-form mask per vector: returned by value, or set bit by
// bit, sample.hip's pass 2 — at its 128-register cap — spills, or beam.hip's pass 1 loses waves of occupancy.)
template <typename T, bool ALIGNED>
__device__ __forceinline__ void load_chunk(const T* p, int V, int base, int lane, float (&v)[SCAN_E], unsigned& out) {
    constexpr int EPV = 16 / sizeof(T);
    out = 0;
#pragma unroll
    for (int j = 0; j < SCAN_E / EPV; ++j) {
        const int i0 = base + (j * 64 + lane) * EPV;
        if constexpr (ALIGNED) {
            if (i0 + EPV <= V) {
                Vec16<T> q = load16<T>(p + i0);
#pragma unroll
                for (int e = 0; e < EPV; ++e) v[j * EPV + e] = q.get(e) + 0.0f;
            } else {  // the row's tail (and what lies behind it)
#pragma unroll
                for (int e = 0; e < EPV; ++e) v[j * EPV + e] = (i0 + e < V) ? to_f32(p[i0 + e]) + 0.0f : -INFINITY;
            }
        } else {
#pragma unroll
            for (int e = 0; e < EPV; ++e) v[j * EPV + e] = (i0 + e < V) ? to_f32(p[i0 + e]) + 0.0f : -INFINITY;
        }
        constexpr unsigned ALL = (1u << EPV) - 1u;
        const int n = V - i0;  // elements of this vector inside the row
        out |= (n >= EPV ? 0u : n <= 0 ? ALL : ALL & ~((1u << n) - 1u)) << (j * EPV);
    }
}

// the chunk's share of the row's softmax, in every lane: (max, sum exp(x - max)) over the wave's 2048 slots
__device__ __forceinline__ float2 chunk_max_sum(const float (&v)[SCAN_E]) {
    float m = -INFINITY;
#pragma unroll
    for (int s = 0; s < SCAN_E; ++s) m = fmaxf(m, v[s]);
    float sum = 0.f;
    if (m != -INFINITY) {
#pragma unroll
        for (int s = 0; s < SCAN_E; ++s) sum += expf(v[s] - m);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float m2 = __shfl_xor(m, off, 64), s2 = __shfl_xor(sum, off, 64);
        const float M = fmaxf(m, m2);
        const float f1 = (m == -INFINITY) ? 0.f : expf(m - M), f2 = (m2 == -INFINITY) ? 0.f : expf(m2 - M);
        sum = sum * f1 + s2 * f2;
        m = M;
    }
    return make_float2(m, sum);
}

// One wave folds a row's chunks ms[0 .. nchunks) into (max, log sum), in every lane: lane-strided, the sum in fp64.
// The row's log-sum-exp is max + log sum; a token's log-probability (x - max) - log sum.
__device__ __forceinline__ float2 fold_chunks(const float2* ms, int nchunks, int lane) {
    float M = -INFINITY;
    for (int c = lane; c < nchunks; c += 64) M = fmaxf(M, ms[c].x);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) M = fmaxf(M, __shfl_xor(M, off, 64));
    double S = 0.0;
    for (int c = lane; c < nchunks; c += 64) {
        const float2 e = ms[c];
        if (e.x != -INFINITY) S += (double)e.y * exp((double)e.x - (double)M);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) S += __shfl_xor(S, off, 64);
    return make_float2(M, S > 0.0 ? (float)log(S) : 0.f);
}

}  // namespace
